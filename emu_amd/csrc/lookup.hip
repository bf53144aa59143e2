// Prompt-lookup speculative greedy decoding: the selection behind a chunk step of T = 1 + k rows (gfx950).
//
//  lookup_argmax : the rows' arg-maxes (lowest index on ties, as argmax_kernel), EOS suppressed in row i while step + i < min_len
//                  with `step` read from the device, so a captured step serves every iteration.
//  lookup_select : ONE workgroup does the rest of the step: accept the draft's leading matches, append the emitted ids to out_ids
//                  and to the history, find the next draft (the first earlier occurrence of the history's last n-gram, longest n
//                  first), advance cur / pos0 / slot0 / ctx / step and the counters.  Integer compares and an integer LDS
//                  minimum only: results repeat bit for bit.  A step at step >= max_new, or after EOS, changes nothing.
//
// What is computed is specified in emu_amd/speculate.py (accept, lookup_draft), which restates transformers'
// PromptLookupCandidateGenerator.get_candidates; the option is lm.generate(prompt_lookup_num_tokens=k), reached through the
// **kwargs of Emu2/emu/emu.py:175,228.
#include "common.h"
#include "kernels.h"

namespace {

__global__ __launch_bounds__(1024) void lookup_argmax_kernel(const LookupArgs a) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    const int r = blockIdx.x, tid = threadIdx.x, vocab = a.V;
    const bf16_t* row = a.logits + (size_t)r * a.ld;
    const int suppress = a.st[LOOKUP_STEP] + r < a.min_len ? a.eos_id : -1;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    auto take = [&](float v, int i) {
        if (i == suppress) v = -INFINITY;
        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
    };
    const int head = (int)((16 - (reinterpret_cast<size_t>(row) & 15)) & 15) >> 1;
    const int h = head < vocab ? head : vocab;
    const int nv = (vocab - h) >> 3;
    if (tid < h) take(bf2f(row[tid]), tid);
    for (int vi = tid; vi < nv; vi += 1024) {
        float f[8];
        unpack8(ld16(row + h + vi * 8), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) take(f[j], h + vi * 8 + j);
    }
    for (int i = h + nv * 8 + tid; i < vocab; i += 1024) take(bf2f(row[i]), i);
    sv[tid] = best; si[tid] = bi;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) {
            const float v = sv[tid + o]; const int i = si[tid + o];
            if (v > sv[tid] || (v == sv[tid] && i < si[tid])) { sv[tid] = v; si[tid] = i; }
        }
        __syncthreads();
    }
    if (tid == 0) a.amax[r] = si[0];
}

__global__ __launch_bounds__(256) void lookup_select_kernel(const LookupArgs a) {
    __shared__ int s_first;                            // the leftmost matching window of the current n
    const int tid = threadIdx.x, k = a.T - 1;
    const int step = a.st[LOOKUP_STEP];
    if (step >= a.max_new || a.st[LOOKUP_FINISHED]) return;        // (uniform) past the end: nothing changes
    // ---- accept: every thread reads the same few words and decides the same
    const int nd = a.st[LOOKUP_NDRAFT], hl = a.st[LOOKUP_HIST_LEN];
    int n = 0;
    while (n < nd && n < k && a.cur[1 + n] == a.amax[n]) ++n;
    int n_emit = n + 1, fin = 0;
    if (n_emit > a.max_new - step) n_emit = a.max_new - step;
    if (a.stop_on_eos)
        for (int i = 0; i < n_emit; ++i)
            if (a.amax[i] == a.eos_id && step + i >= a.min_len) { n_emit = i + 1; fin = 1; break; }
    const int now = step + n_emit, L = hl + n_emit;
    if (now >= a.max_new) fin = 1;
    const int mine = tid < n_emit ? a.amax[tid] : 0, last_id = a.amax[n_emit - 1];
    __syncthreads();                                   // everyone has read cur / amax / st: they are rewritten from here on
    if (tid < n_emit) {
        a.out_ids[step + tid] = mine;
        if (hl + tid < a.hist_cap) a.hist[hl + tid] = mine;
    }
    __syncthreads();                                   // the history's new tail is visible to the workgroup
    // ---- the next draft: up to k ids behind the leftmost earlier occurrence of the last n ids, longest n first
    int start = -1, ndn = 0;
    if (!fin && a.drafts) { ndn = k; }
    else if (!fin && L <= a.hist_cap) {
        for (int ng = a.max_ngram < L - 1 ? a.max_ngram : L - 1; ng >= 1 && start < 0; --ng) {
            if (tid == 0) s_first = 0x7fffffff;
            __syncthreads();
            for (int i = tid; i + ng < L; i += 256) {  // a window that is followed by at least one id
                bool eq = true;
                for (int j = 0; j < ng; ++j) eq = eq && a.hist[i + j] == a.hist[L - ng + j];
                if (eq) atomicMin(&s_first, i);
            }
            __syncthreads();
            if (s_first != 0x7fffffff) start = s_first + ng;
            __syncthreads();                           // (s_first is reset by the next n)
        }
        if (start >= 0) ndn = L - start < k ? L - start : k;
    }
    if (tid < k) {
        int id = 0;                                    // rows beyond the draft carry id 0 and are never accepted
        if (tid < ndn) id = a.drafts ? a.drafts[(size_t)now * k + tid] : a.hist[start + tid];
        if (!fin) a.cur[1 + tid] = id;
    }
    if (tid == 0) {
        if (!fin) a.cur[0] = last_id;
        a.st[LOOKUP_STEP] = now;
        a.st[LOOKUP_FINISHED] = fin;
        a.st[LOOKUP_NDRAFT] = ndn;
        a.st[LOOKUP_HIST_LEN] = L;
        a.st[LOOKUP_STEPS_RUN] += 1;
        a.st[LOOKUP_EMITTED] += n_emit;
        *a.pos0 += n_emit; *a.slot0 += n_emit; *a.ctx += n_emit;
    }
}

bool lookup_args_ok(const LookupArgs& a) {
    return a.logits && a.amax && a.cur && a.st && a.pos0 && a.slot0 && a.ctx && a.out_ids && a.hist && a.T >= 2 &&
           a.T <= DECODE_CHUNK_MAX && a.V >= 1 && a.max_new >= 1 && a.max_ngram >= 1 && a.hist_cap >= 1;
}

}  // namespace

int launch_lookup_argmax(const LookupArgs& a, hipStream_t s) {
    if (!lookup_args_ok(a)) return -22;
    hipLaunchKernelGGL(lookup_argmax_kernel, dim3(a.T), dim3(1024), 0, s, a);
    EMU_CHECK_LAUNCH();
    return 0;
}

int launch_lookup_select(const LookupArgs& a, hipStream_t s) {
    if (!lookup_args_ok(a)) return -22;
    hipLaunchKernelGGL(lookup_select_kernel, dim3(1), dim3(256), 0, s, a);
    EMU_CHECK_LAUNCH();
    return 0;
}
