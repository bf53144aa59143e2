// The no-repeat n-gram ban on the device (transformers' NoRepeatNGramLogitsProcessor; the reference hands no_repeat_ngram_size to
// lm.generate, Emu1/models/modeling_emu.py:115,177): the match loop the selection kernels share (sample.hip, beam_sample.hip,
// beam.hip).  The specification is emu_amd/sampling.py::banned_ngram_mask: with h[0 .. nh) the ids a row has generated, id v is
// banned iff nh + 1 >= n and some i in [0, nh - n + 1) has h[i .. i + n - 1) == h[nh - n + 1 .. nh) and h[i + n - 1] == v.
// Every read lies in [0, nh): the caller bounds nh by the rows its history holds; what is done with a banned id -- its range check
// included -- is the caller's.
#pragma once
#include "common.h"

namespace {

// Calls emit(id) for every start position i = tid, tid + nthreads, ... whose n - 1 ids equal the last n - 1 of the history
// (n = 1: every position), id = h[(i + n - 1) * stride] the id that completed the n-gram there.  h[t * stride] is id t.
template <class Emit>
__device__ __forceinline__ void ngram_matches(const int32_t* h, size_t stride, int nh, int n, int tid, int nthreads, Emit emit) {
    if (n < 1 || nh + 1 < n) return;
    const int tail = nh - (n - 1);                     // the last n - 1 ids start here; start positions are [0, tail)
    for (int i = tid; i < tail; i += nthreads) {
        bool same = true;
        for (int k = 0; k < n - 1 && same; ++k) same = h[(size_t)(i + k) * stride] == h[(size_t)(tail + k) * stride];
        if (same) emit(h[(size_t)(i + n - 1) * stride]);
    }
}

}  // namespace
