// One step of transformers' beam-search multinomial sampling (lm.generate(num_beams=N, do_sample=True, temperature, top_k, top_p,
// repetition_penalty): the call of the reference's demo backend, demo/backend/pytorch_model/backend.py:179-186) and of penalised
// beam search (do_sample=False with a repetition penalty), on the device, in two launches.  The specification is
// emu_amd/sampling.py (beam_reference_rows / beam_reference_probs / beam_reference_select); the deterministic, unpenalised step stays
// beam.hip's.
//   A. beam_rows_kernel, one workgroup of 1024 threads per beam row (sample_common.h's row-in-LDS machinery): lp = x - logsumexp(x),
//      repetition penalty over the beam's own ids (running_seq[b, j, :cur]), EOS -> -inf while cur < min_len, then the warpers
//      (temperature, top-k, top-p, min_keep >= 2) on lp ("5.x" order, the running score added afterwards) or on lp + running score
//      ("4.31" order).  To the workspace: the accumulated score of every id (-inf = removed), exp(acc - row maximum), the row maximum.
//   B. beam_draw_kernel, one workgroup of 1024 threads per prompt: the rows' masses under the common maximum, then 2N draws
//      without replacement, each from one uniform: the row by cumulative row mass, inside the row the owning thread chunk by a
//      block-wide scan of the chunk sums, then the id by a sequential walk -- every sum in a fixed order, a drawn entry's mass set to
//      zero and its chunk sum rebuilt (never subtracted: no drift).  When no mass remains (the "5.x" start: beams 1..N-1 carry -1e9)
//      the draw takes the lowest flat index not yet drawn whose score is finite.  do_sample = 0: 2N arg-max rounds under before()
//      instead.  The "4.31" order then sorts the draws by score (stable), and beam_common.h's bookkeeping runs as in beam.hip.
// Both kernels read the step index from the device counter when one is given and return at once from the length limit on, so a
// captured hipGraph replays the step for every token.
// With a no-repeat n-gram ban (emu_beam_sample_step_ngram_bf16; BeamStepArgs::ngram > 0; ngram.h) kernel A writes -inf over the id
// behind every earlier occurrence of the beam's last n - 1 ids, between the penalty and the EOS suppress, as sample.hip does.
#include "beam_common.h"
#include "sample_common.h"
#include "ngram.h"

namespace {

constexpr int NONE = 0x7fffffff;

__global__ __launch_bounds__(SAMPLE_THREADS) void beam_rows_kernel(const BeamSampleArgs a, float* ws) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* sf = reinterpret_cast<float*>(lds_raw);               // 192 words of reduction scratch
    int* si = reinterpret_cast<int*>(lds_raw) + 64;
    uint32_t* keys = reinterpret_cast<uint32_t*>(lds_raw + SAMPLE_SCRATCH);
    float* score = reinterpret_cast<float*>(keys);               // the same words hold fp32 scores until the keys are made

    const BeamStepArgs& st = a.st;
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, V = st.V, nb = st.nb;
    const int cur = st.cur_dev ? *st.cur_dev : st.cur;
    if (cur >= st.L) return;                                     // graph replays beyond the length limit are no-ops
    const size_t row = (size_t)b * nb + j;
    const bf16_t* lrow = st.logits + (size_t)b * st.ld_prompt + (size_t)j * st.ld_beam;
    const float rs = st.running_scores[row];
    float* acc_w = ws + row * V;
    float* e_w = ws + ((size_t)st.B * nb + row) * V;
    float* acc_o = a.acc_out ? a.acc_out + row * a.ld_acc : nullptr;

    load_row_scores(lrow, V, score);
    __syncthreads();
    int C = (V + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
    C |= 1;
    const int i0 = tid * C;
    const int n = i0 >= V ? 0 : (V - i0 < C ? V - i0 : C);       // ids this thread owns: [i0, i0 + n)

    // 1. lp = x - (m + log sum exp(x - m)): blocked sum
    float m = -INFINITY;
    for (int q = 0; q < n; ++q) m = fmaxf(m, score[i0 + q]);
    m = block_max_f(m, sf);
    float z[1] = {0.f};
    for (int q = 0; q < n; ++q) z[0] += expf(score[i0 + q] - m);
    block_sum_f<1>(z, sf);
    const float lse = m + logf(z[0]);
    for (int q = 0; q < n; ++q) score[i0 + q] = score[i0 + q] - lse;
    __syncthreads();
    // 2. repetition penalty, once per distinct id: every occurrence writes the same value computed from the ORIGINAL logit
    if (a.penalty != 1.0f) {
        const int32_t* hist = st.running_seq + row * st.L;
        for (int t = tid; t < cur; t += SAMPLE_THREADS) {
            const int id = hist[t];
            if (id >= 0 && id < V) {
                const float s = bf2f(lrow[id]) - lse;
                score[id] = s < 0.f ? s * a.penalty : s / a.penalty;
            }
        }
        __syncthreads();
    }
    // 2a. no-repeat n-gram ban over the beam's own ids
    if (st.ngram > 0) {
        ngram_matches(st.running_seq + row * st.L, 1, cur, st.ngram, tid, SAMPLE_THREADS, [&](int id) {
            if (id >= 0 && id < V) score[id] = -INFINITY;
        });
        __syncthreads();
    }
    if (st.eos_id >= 0 && st.eos_id < V && cur < st.min_len) {
        if (tid == 0) score[st.eos_id] = -INFINITY;
        __syncthreads();
    }

    // penalised beam search: no warpers, acc = lp + running score
    if (!a.do_sample) {
        for (int q = 0; q < n; ++q) {
            const float v = score[i0 + q] + rs;
            acc_w[i0 + q] = v;
            if (acc_o) acc_o[i0 + q] = v;
        }
        return;
    }

    // 3. the warpers' input (the running score on the side the order names), temperature, -0 -> +0, scores -> keys in place
    const bool accumulated = a.warp_accumulated != 0;
    float mx = -INFINITY;
    const bool scale = a.temperature != 1.0f;
#pragma unroll
    for (int q = 0; q < SAMPLE_CMAX; ++q) {
        if (q < n) {
            float s = score[i0 + q];
            if (accumulated) s = s + rs;
            if (scale) s = s / a.temperature;
            if (s == 0.f) s = 0.f;
            mx = fmaxf(mx, s);
            keys[i0 + q] = f2key(s);
        }
    }
    mx = block_max_f(mx, sf);
    float p[SAMPLE_CMAX];
    const uint32_t t_keep = warp_threshold(keys, p, i0, n, V, mx, a.top_k, a.top_p, a.min_keep, sf, si);

    // 4. acc and its mass under the row maximum (rounding is monotone: the maximum of acc is the image of the maximum score)
    const float amax = accumulated ? mx : mx + rs;
#pragma unroll
    for (int q = 0; q < SAMPLE_CMAX; ++q) {
        if (q < n) {
            const uint32_t k = keys[i0 + q];
            const float s = key2f(k);
            const float v = k >= t_keep ? (accumulated ? s : s + rs) : -INFINITY;
            acc_w[i0 + q] = v;
            e_w[i0 + q] = v == -INFINITY ? 0.f : expf(v - amax);
            if (acc_o) acc_o[i0 + q] = v;
        }
    }
    if (tid == 0) ws[2 * (size_t)st.B * nb * V + row] = amax;
}

__global__ __launch_bounds__(SAMPLE_THREADS) void beam_draw_kernel(const BeamSampleArgs a, float* ws) {
    __shared__ float sf[64];
    __shared__ int si[64];
    __shared__ int found[2];                           // [0] lowest id past the draw, [1] highest id of positive mass
    __shared__ float top_lp[2 * BEAM_MAXN];
    __shared__ int top_idx[2 * BEAM_MAXN];
    __shared__ float s_scale[BEAM_MAXN], s_sum[BEAM_MAXN];
    __shared__ float pre[BEAM_MAXN][SAMPLE_THREADS];   // per row: sum of the chunk sums of the threads before this one

    const BeamStepArgs& st = a.st;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, V = st.V, nb = st.nb, T = 2 * nb;
    const int cur = st.cur_dev ? *st.cur_dev : st.cur;
    if (cur >= st.L) return;
    const float* acc_w = ws + (size_t)b * nb * V;
    float* e_w = ws + ((size_t)st.B * nb + (size_t)b * nb) * V;
    const float* rmax = ws + 2 * (size_t)st.B * nb * V + (size_t)b * nb;
    int C = (V + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
    C |= 1;
    const int i0 = tid * C;
    const int n = i0 >= V ? 0 : (V - i0 < C ? V - i0 : C);       // ids of every row this thread owns: [i0, i0 + n)

    if (a.do_sample) {
        float M = -INFINITY;
        for (int j = 0; j < nb; ++j) M = fmaxf(M, rmax[j]);
        if (tid < nb) s_scale[tid] = expf(rmax[tid] - M);
        float cs[BEAM_MAXN];                           // this thread's chunk sum of every row (ascending ids)
#pragma unroll
        for (int j = 0; j < BEAM_MAXN; ++j) {
            cs[j] = 0.f;
            if (j < nb) {
                for (int q = 0; q < n; ++q) cs[j] += e_w[(size_t)j * V + i0 + q];
                float total;
                pre[j][tid] = block_scan_f(cs[j], total, sf);
                if (tid == 0) s_sum[j] = total;
            }
        }
        int urow = cur < a.uni_rows ? cur : a.uni_rows - 1;
        if (urow < 0) urow = 0;
        const float* u = a.uniforms + ((size_t)urow * st.B + b) * T;
        for (int k = 0; k < T; ++k) {
            __syncthreads();                           // s_sum / pre / top_idx of the draw before
            if (tid == 0) { found[0] = NONE; found[1] = -1; }
            // the row: lowest j of positive mass whose inclusive cumulative mass exceeds u * R, else the last of positive mass
            float R = 0.f, cb = 0.f, cb_last = 0.f;
            int jsel = -1, jlast = -1;
            for (int j = 0; j < nb; ++j) R += s_scale[j] * s_sum[j];
            const float target = u[k] * R;
            {
                float c = 0.f;
                for (int j = 0; j < nb; ++j) {
                    const float w = s_scale[j] * s_sum[j];
                    if (w > 0.f) {
                        jlast = j; cb_last = c;
                        if (jsel < 0 && c + w > target) { jsel = j; cb = c; }
                    }
                    c += w;
                }
            }
            if (jsel < 0) { jsel = jlast; cb = cb_last; }
            __syncthreads();                           // found is reset
            int hit = NONE, hi = -1;
            if (jsel >= 0) {
                // inside the row: cumulative mass of id i0 + q = cb + scale * (the chunks before + the chunk's own sequential prefix)
                const float sc = s_scale[jsel], base = pre[jsel][tid];
                const float* e = e_w + (size_t)jsel * V + i0;
                float lp = 0.f;
                for (int q = 0; q < n; ++q) {
                    const float v = e[q];
                    if (v > 0.f) {
                        lp += v;
                        hi = i0 + q;
                        if (hit == NONE && cb + sc * (base + lp) > target) hit = i0 + q;
                    }
                }
            } else {
                // no mass remains: the lowest flat index not yet drawn whose score is finite
                for (int j = 0; j < nb && hit == NONE; ++j)
                    for (int q = 0; q < n && hit == NONE; ++q) {
                        const int idx = j * V + i0 + q;
                        bool drawn = false;
                        for (int d = 0; d < k; ++d) drawn |= top_idx[d] == idx;
                        if (!drawn && acc_w[idx] != -INFINITY) hit = idx;
                    }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                hit = min(hit, __shfl_xor(hit, o));
                hi = max(hi, __shfl_xor(hi, o));
            }
            if (lane == 0) {
                if (hit != NONE) atomicMin(&found[0], hit);
                if (hi >= 0) atomicMax(&found[1], hi);
            }
            __syncthreads();
            int flat;
            if (jsel >= 0) {
                int tok = found[0] != NONE ? found[0] : found[1];    // rounding left the target at or beyond the row's total
                if (tok < 0 || tok >= V) tok = 0;
                flat = jsel * V + tok;
                if (tok >= i0 && tok < i0 + n) e_w[flat] = 0.f;      // its owner retires it and rebuilds the chunk sum
                float total = 0.f;
#pragma unroll
                for (int j = 0; j < BEAM_MAXN; ++j) {
                    if (j == jsel) {
                        if (tok >= i0 && tok < i0 + n) {
                            cs[j] = 0.f;
                            for (int q = 0; q < n; ++q) cs[j] += e_w[(size_t)j * V + i0 + q];
                        }
                        pre[j][tid] = block_scan_f(cs[j], total, sf);
                    }
                }
                if (tid == 0) s_sum[jsel] = total;
            } else {
                flat = found[0] != NONE ? found[0] : 0;
            }
            if (tid == 0) {
                top_idx[k] = flat;
                top_lp[k] = acc_w[flat];
                if (a.draws_out) a.draws_out[(size_t)b * T + k] = flat;
            }
        }
        __syncthreads();
        // the "4.31" order ranks its draws before the scorer sees them (stable: equal scores keep draw order)
        if (tid == 0 && a.warp_accumulated) {
            for (int k = 1; k < T; ++k) {
                const float v = top_lp[k];
                const int i = top_idx[k];
                int q = k;
                while (q > 0 && top_lp[q - 1] < v) { top_lp[q] = top_lp[q - 1]; top_idx[q] = top_idx[q - 1]; --q; }
                top_lp[q] = v; top_idx[q] = i;
            }
        }
    } else {
        // the 2N best of beams x vocabulary under before(): every thread keeps the best entry it has not yet given away and looks
        // for its next one only after a win
        float pv = INFINITY; int pi = -1;              // last pick (everything taken ranks before or at it)
        float mv = -INFINITY; int mi = NONE;
        bool look = true;
        for (int k = 0; k < T; ++k) {
            if (look) {
                mv = -INFINITY; mi = NONE;
                for (int j = 0; j < nb; ++j)
                    for (int q = 0; q < n; ++q) {
                        const int idx = j * V + i0 + q;
                        const float x = acc_w[idx];
                        const bool taken = pi >= 0 && !before(pv, pi, x, idx);
                        if (!taken && before(x, idx, mv, mi)) { mv = x; mi = idx; }
                    }
                look = false;
            }
            float bv = mv; int bi = mi;
            block_argmax_first(bv, bi, sf, si);
            if (bi == NONE) bi = 0;                    // (not reached: V >= 2N entries per row)
            if (tid == 0) {
                top_lp[k] = bv; top_idx[k] = bi;
                if (a.draws_out) a.draws_out[(size_t)b * T + k] = bi;
            }
            pv = bv; pi = bi;
            look = bi == mi;
        }
    }
    __syncthreads();
    beam_bookkeeping<SAMPLE_THREADS>(st, b, cur, top_lp, top_idx);
}

}  // namespace

size_t beam_sample_ws_floats(int B, int nb, int V) { return (size_t)B * nb * (2 * (size_t)V + 1); }

int launch_beam_sample_step(const BeamSampleArgs& a, float* ws, size_t ws_floats, hipStream_t s) {
    const BeamStepArgs& st = a.st;
    if (st.B < 1 || st.nb < 1 || st.nb > BEAM_MAXN || st.L < 1 || st.L > BEAM_MAXL || (!st.cur_dev && (st.cur < 0 || st.cur >= st.L)) ||
        st.V > EMU_SAMPLE_MAX_VOCAB || st.V < 2 * st.nb || st.min_len < 0 || !ws || ws_floats < beam_sample_ws_floats(st.B, st.nb, st.V))
        return -22;
    if (!(a.penalty > 0.f) || (a.acc_out && a.ld_acc < st.V) || st.ngram < 0) return -22;
    if (a.do_sample && (!a.uniforms || a.uni_rows < 1 || !(a.temperature > 0.f) || !(a.top_p > 0.f) || a.min_keep < 2)) return -22;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(beam_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                SAMPLE_SCRATCH + EMU_SAMPLE_MAX_VOCAB * 4) != hipSuccess)
            return -5;
        attr_set = true;
    }
    const size_t lds = SAMPLE_SCRATCH + (((size_t)st.V * 4 + 15) & ~(size_t)15);
    hipLaunchKernelGGL(beam_rows_kernel, dim3(st.nb, st.B), dim3(SAMPLE_THREADS), lds, s, a, ws);
    hipLaunchKernelGGL(beam_draw_kernel, dim3(st.B), dim3(SAMPLE_THREADS), 0, s, a, ws);
    EMU_CHECK_LAUNCH();
    return 0;
}
