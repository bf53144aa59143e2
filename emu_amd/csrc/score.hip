// The log-probability of a FORCED token under a row of logits, in one launch (the specification is emu_amd/scoring.py): per row the
// log-sum-exp, lp = x[t] - lse for the row's target t, the first-index arg-max, and -- with a second row r of reference logits --
// KL(softmax r || softmax x) and whether the two arg-maxes agree.  It is what the reference's LM loss needs per position
// (Emu1/models/modeling_llama.py:110-116: CrossEntropyLoss over shifted logits / labels) and what prediction_mixin.py:36-131 ranks
// candidate answers by; the quantised weight streams are evaluated with it (tools/quant_eval.py).
//
// One workgroup of 1024 threads per row.  The row is STREAMED from memory, never held in LDS, so there is no vocabulary bound: a
// 32 274-token row is 64 KB, read once from HBM (or from the L2 the head's GEMM left it in) and again from L2 by the later passes.
// Thread t owns the contiguous ids [t * C, t * C + C), C = ceil(V / 1024) rounded up to a multiple of 8, and walks them in ascending
// id order: scalar loads up to the first 16-byte boundary, 16-byte loads over the aligned body, scalar loads over the tail -- any
// 2-byte-aligned base is accepted (the vocabulary-sharded head hands out odd element offsets), and ownership does not depend on the
// alignment, so neither does any result.
//
// The passes:   1. m = max x and the first index of it (and the same of r);
//               2. Z = sum exp(x - m) (and of r);  lse = m + log Z;
//               3. (with r) kl = sum p_r * (logp_r - logp_x), logp = x - lse, p_r = exp(logp_r), terms with p_r == 0 left out.
// The order of every sum is part of the specification: each thread adds its <= C terms sequentially in fp32 in ascending id order,
// then sample_common.h's fixed tree (6 levels inside the wave, 4 across the 16 waves).  No floating-point atomics: the same inputs
// give the same bits on every launch.
//
// The target of row r is targets[step * tgt_ld + r] and every output goes to out[step * out_ld + r], step = *step_dev (0 without
// one): the step is never a host scalar, so one captured graph serves every step of a teacher-forced loop (emu_llama_score_step).
#include "sample_common.h"

namespace {

struct ScoreArgs {
    const bf16_t* logits; int ld; int vocab;
    const int32_t* targets; int tgt_ld;
    const int32_t* step; int limit;                              // limit > 0: the launch does nothing once *step >= limit
    const bf16_t* ref; int ref_ld;
    float* lp; float* lse; int32_t* top1; float* kl; int32_t* agree; int out_ld;
    int32_t* force;                                              // force[row] = the target, 0 for an ignored one (the step's next input)
};

// f(id, x) -- or f(id, x, r) with a reference row -- over the ids [i0, i0 + n) in ascending order
template <bool REF, typename F>
__device__ __forceinline__ void walk_chunk(const bf16_t* x, const bf16_t* r, int i0, int n, F&& f) {
    const int head = (int)((16 - (reinterpret_cast<size_t>(x + i0) & 15)) & 15) >> 1;
    const int h = head < n ? head : n;
    const int nv = (n - h) >> 3;
    // the reference row may sit at another alignment: its body is loaded 16 bytes at a time only where it is aligned as well
    const bool rvec = REF && ((reinterpret_cast<size_t>(r + i0 + h) & 15) == 0);
    int i = i0;
    for (; i < i0 + h; ++i) f(i, bf2f(x[i]), REF ? bf2f(r[i]) : 0.f);
    for (int v = 0; v < nv; ++v, i += 8) {
        float fx[8], fr[8];
        unpack8(ld16(x + i), fx);
        if (REF) {
            if (rvec) unpack8(ld16(r + i), fr);
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j) fr[j] = bf2f(r[i + j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) f(i + j, fx[j], REF ? fr[j] : 0.f);
    }
    for (; i < i0 + n; ++i) f(i, bf2f(x[i]), REF ? bf2f(r[i]) : 0.f);
}

template <bool REF>
__global__ __launch_bounds__(SAMPLE_THREADS) void token_logprob_kernel(ScoreArgs a) {
    __shared__ float sf[2 * SAMPLE_WAVES];                       // every read of the scratch is a broadcast: no bank conflicts
    __shared__ int si[SAMPLE_WAVES];
    const int step = a.step ? *a.step : 0;
    if (a.limit > 0 && step >= a.limit) return;
    const int row = blockIdx.x, tid = threadIdx.x, V = a.vocab;
    const bf16_t* x = a.logits + (size_t)row * a.ld;
    const bf16_t* r = REF ? a.ref + (size_t)row * a.ref_ld : nullptr;

    const int C = (((V + SAMPLE_THREADS - 1) / SAMPLE_THREADS) + 7) & ~7;
    const long long first = (long long)tid * C;
    const int i0 = first < V ? (int)first : V;
    const int n = V - i0 < C ? V - i0 : C;                       // ids this thread owns: [i0, i0 + n)

    // 1. maxima and their first indices
    float mx = -INFINITY, mr = -INFINITY;
    int ix = 0x7fffffff, ir = 0x7fffffff;
    walk_chunk<REF>(x, r, i0, n, [&](int i, float vx, float vr) {
        if (vx > mx) { mx = vx; ix = i; }                        // ascending ids, strict: the first index of a tie stays
        if (REF && vr > mr) { mr = vr; ir = i; }
    });
    block_argmax_first(mx, ix, sf, si);
    if (REF) block_argmax_first(mr, ir, sf, si);
    if (ix >= V) ix = 0;                                         // a row of NaNs or of -inf alone: argmax_kernel's answer
    if (REF && ir >= V) ir = 0;

    // 2. Z = sum exp(x - m)
    float z[2] = {0.f, 0.f};
    walk_chunk<REF>(x, r, i0, n, [&](int, float vx, float vr) {
        z[0] += expf(vx - mx);
        if (REF) z[1] += expf(vr - mr);
    });
    block_sum_f<REF ? 2 : 1>(z, sf);
    const float lse = mx + logf(z[0]);
    const float lser = REF ? mr + logf(z[1]) : 0.f;

    // 3. KL(ref || x)
    float kl[1] = {0.f};
    if (REF && a.kl) {
        walk_chunk<REF>(x, r, i0, n, [&](int, float vx, float vr) {
            const float lpr = vr - lser;
            const float pr = expf(lpr);
            if (pr != 0.f) kl[0] += pr * (lpr - (vx - lse));
        });
        block_sum_f<1>(kl, sf);
    }

    if (tid == 0) {
        const size_t o = (size_t)step * a.out_ld + row;
        const int t = a.targets[(size_t)step * a.tgt_ld + row];
        const bool counted = t >= 0 && t < V;
        if (a.lp) a.lp[o] = counted ? bf2f(x[t]) - lse : 0.f;
        if (a.lse) a.lse[o] = lse;
        if (a.top1) a.top1[o] = ix;
        if (REF && a.kl) a.kl[o] = kl[0];
        if (REF && a.agree) a.agree[o] = ix == ir ? 1 : 0;
        if (a.force) a.force[row] = counted ? t : 0;
    }
}

}  // namespace

int launch_token_logprob(const bf16_t* logits, int ld, int rows, int vocab, const int32_t* targets, int tgt_ld, const int32_t* step_dev,
                         int limit, const bf16_t* ref_logits, int ref_ld, float* lp, float* lse, int32_t* top1, float* kl,
                         int32_t* agree, int out_ld, int32_t* force_ids, hipStream_t s) {
    if (!logits || !targets || rows < 1 || vocab < 1 || ld < vocab || tgt_ld < rows || out_ld < rows) return -22;
    if (ref_logits && ref_ld < vocab) return -22;
    ScoreArgs a;
    a.logits = logits; a.ld = ld; a.vocab = vocab;
    a.targets = targets; a.tgt_ld = tgt_ld;
    a.step = step_dev; a.limit = limit;
    a.ref = ref_logits; a.ref_ld = ref_ld;
    a.lp = lp; a.lse = lse; a.top1 = top1; a.kl = kl; a.agree = agree; a.out_ld = out_ld;
    a.force = force_ids;
    if (ref_logits) hipLaunchKernelGGL(token_logprob_kernel<true>, dim3(rows), dim3(SAMPLE_THREADS), 0, s, a);
    else hipLaunchKernelGGL(token_logprob_kernel<false>, dim3(rows), dim3(SAMPLE_THREADS), 0, s, a);
    EMU_CHECK_LAUNCH();
    return 0;
}
