// What the beam-step kernels share (beam.hip: the deterministic step; beam_sample.hip: beam-search sampling and penalised beam
// search): the limits, the ranking rule, and the scorer's bookkeeping, so that its rules are written once.
#pragma once
#include "common.h"
#include "kernels.h"

namespace {

constexpr int BEAM_MAXN = 8;                           // beams per prompt
constexpr int BEAM_MAXL = 256;                         // generated tokens
constexpr float BEAM_NEG = -1.0e9f;

// "a ranks before b": higher value first, then lower index
__device__ __forceinline__ bool before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// The scorer's bookkeeping of prompt b at step cur, statement for statement the host's (emu_amd/llama.py::beam_search_generate), by
// the whole workgroup of NT threads: top_lp / top_idx (LDS, 2N entries, visible to every thread) are the step's candidates in the scorer's order,
// top_idx = beam * V + token.  The N best non-finished candidates keep running, the finished ones among the first N compete with the
// kept results, the early-stopping heuristic is updated, the state and the step's outputs are written.
template <int NT>
__device__ __forceinline__ void beam_bookkeeping(const BeamStepArgs& a, int b, int cur, const float* top_lp, const int* top_idx) {
    __shared__ int cand[2 * BEAM_MAXN][BEAM_MAXL];     // candidate sequences
    __shared__ int kept[BEAM_MAXN][BEAM_MAXL];         // kept results before this step
    const int tid = threadIdx.x;
    const int nb = a.nb, V = a.V, L = a.L;
    int* run_seq = a.running_seq + (size_t)b * nb * L;
    int* res_seq = a.sequences + (size_t)b * nb * L;
    float* run_sc = a.running_scores + (size_t)b * nb;
    float* res_sc = a.beam_scores + (size_t)b * nb;
    unsigned char* fin = a.finished + (size_t)b * nb;
    int* res_len = a.seq_len + (size_t)b * nb;
    // Stage the candidate sequences and the kept results, then one thread decides, then all write back.
    const int n2 = 2 * nb;
    for (int q = tid; q < n2 * L; q += NT) {
        const int k = q / L, p = q - k * L;
        const int src = top_idx[k] / V;
        cand[k][p] = p == cur ? top_idx[k] - src * V : run_seq[src * L + p];
    }
    for (int q = tid; q < nb * L; q += NT) kept[q / L][q % L] = res_seq[q];
    __shared__ int nxt[BEAM_MAXN], keep[BEAM_MAXN];
    __shared__ float new_rs[BEAM_MAXN], new_sc[BEAM_MAXN];
    __shared__ int new_len[BEAM_MAXN];
    __shared__ unsigned char new_fin[BEAM_MAXN];
    __syncthreads();
    if (tid == 0) {
        bool hits[2 * BEAM_MAXN];
        float run_lp[2 * BEAM_MAXN], fin_lp[2 * BEAM_MAXN];
        const bool open = a.heuristic_open[b] != 0;
        const bool v431 = a.hf431 != 0, at_limit = cur + 1 >= L;
        // (cur + 1) ** length_penalty as the host's double-precision power rounded to fp32 (the torch pipeline's divisor)
        const float len_div = (float)pow((double)(cur + 1), (double)a.length_penalty);
        const float eos_div = (v431 && cur > 0) ? (float)pow((double)cur, (double)a.length_penalty) : len_div;
        for (int k = 0; k < n2; ++k) {
            const int tok = top_idx[k] % V;
            const bool eos = tok == a.eos_id;
            hits[k] = eos || (!v431 && at_limit);      // 4.31: at the limit the non-EOS candidates still become running beams
            run_lp[k] = top_lp[k] + (hits[k] ? 1.f : 0.f) * BEAM_NEG;
            float f = top_lp[k] / (eos ? eos_div : len_div);
            f = f + (open ? 0.f : 1.f) * BEAM_NEG;
            const bool just = hits[k] && k < nb;       // only the first N candidates may finish
            f = f + (just ? 0.f : 1.f) * BEAM_NEG;
            fin_lp[k] = f;
        }
        // the N best running candidates (stable: equal scores keep candidate order)
        bool used[2 * BEAM_MAXN] = {};
        for (int j = 0; j < nb; ++j) {
            int best = -1;
            for (int k = 0; k < n2; ++k)
                if (!used[k] && (best < 0 || run_lp[k] > run_lp[best])) best = k;
            used[best] = true;
            nxt[j] = best;
            new_rs[j] = run_lp[best];
        }
        // merge the finished candidates with the kept results: N best of (kept 0..N-1, candidates 0..2N-1)
        bool usedm[3 * BEAM_MAXN] = {};
        for (int j = 0; j < nb; ++j) {
            int best = -1; float bs = 0.f;
            for (int e = 0; e < nb + n2; ++e) {
                if (usedm[e]) continue;
                const float sc = e < nb ? res_sc[e] : fin_lp[e - nb];
                if (best < 0 || sc > bs) { best = e; bs = sc; }
            }
            usedm[best] = true;
            keep[j] = best;
            new_sc[j] = bs;
            new_fin[j] = best < nb ? fin[best] : (unsigned char)(hits[best - nb] && best - nb < nb);
            new_len[j] = best < nb ? res_len[best] : cur + 1;
        }
        // early-stopping heuristic (early_stopping=False): can the best running beam (4.31: the best of all 2N candidates, an
        // EOS one included) still beat the worst kept result?
        const float best_run = (v431 ? top_lp[0] : new_rs[0]) / len_div;
        float worst = INFINITY;
        for (int j = 0; j < nb; ++j) worst = fminf(worst, new_sc[j]);
        bool still = false;
        for (int j = 0; j < nb; ++j) still |= best_run > (new_fin[j] ? worst : BEAM_NEG);
        const bool open_now = open && still;
        a.heuristic_open[b] = (unsigned char)open_now;
        // 4.31 `finalize` at the length limit: the N running beams (now L tokens long) join the kept results at L ** length_penalty
        // unless the prompt is done; entries nb + n2 + j of the merge below are running beam j (= candidate nxt[j])
        if (v431 && at_limit) {
            float k_sc[BEAM_MAXN]; int k_src[BEAM_MAXN]; int k_len[BEAM_MAXN]; unsigned char k_fin[BEAM_MAXN];
            for (int j = 0; j < nb; ++j) { k_sc[j] = new_sc[j]; k_src[j] = keep[j]; k_len[j] = new_len[j]; k_fin[j] = new_fin[j]; }
            bool used2[2 * BEAM_MAXN] = {};
            for (int j = 0; j < nb; ++j) {
                int best = -1; float bs = 0.f;
                for (int e = 0; e < 2 * nb; ++e) {
                    if (used2[e]) continue;
                    const float sc = e < nb ? k_sc[e] : new_rs[e - nb] / len_div + (open_now ? 0.f : 1.f) * BEAM_NEG;
                    if (best < 0 || sc > bs) { best = e; bs = sc; }
                }
                used2[best] = true;
                new_sc[j] = bs;
                if (best < nb) { keep[j] = k_src[best]; new_fin[j] = k_fin[best]; new_len[j] = k_len[best]; }
                else { keep[j] = nb + nxt[best - nb]; new_fin[j] = 1; new_len[j] = cur + 1; }
            }
        }
    }
    __syncthreads();
    for (int q = tid; q < nb * L; q += NT) {
        const int j = q / L, p = q - j * L;
        run_seq[q] = cand[nxt[j]][p];
        const int e = keep[j];
        res_seq[q] = e < nb ? kept[e][p] : cand[e - nb][p];
    }
    if (tid < nb) {
        run_sc[tid] = new_rs[tid];
        res_sc[tid] = new_sc[tid];
        fin[tid] = new_fin[tid];
        res_len[tid] = new_len[tid];
        a.next_tok[b * nb + tid] = cand[nxt[tid]][cur];
        a.beam_flat[b * nb + tid] = (long)b * nb + top_idx[nxt[tid]] / V;
    }
}

}  // namespace
