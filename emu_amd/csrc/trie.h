// Constrained decoding on the device: reading the flat token trie (include/emu_hip.h: emu_token_trie; emu_amd/constrain.py builds it)
// from the selection kernels (sample.hip, beam.hip).  Every table value is clamped before it becomes an address: a node outside
// [0, nodes) is "exhausted" (only EOS is allowed), an edge range is cut to [0, edges].
#pragma once
#include "common.h"
#include "kernels.h"

namespace {

// the edge range [lo, hi) of `node`; false (and an empty range) for the exhausted node -- out of range, or without edges
__device__ __forceinline__ bool trie_edges(const emu_token_trie& t, int node, int& lo, int& hi) {
    lo = hi = 0;
    if (node < 0 || node >= t.nodes) return false;
    lo = t.first[node];
    hi = t.first[node + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > t.edges ? t.edges : hi;
    return lo < hi;
}

// first edge in [lo, hi) whose id is >= id (hi when there is none): the ids of a node ascend
__device__ __forceinline__ int trie_lower_bound(const int32_t* tok, int lo, int hi, int id) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (tok[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the node after `id` at `node`: -1 when id is no edge of it
__device__ __forceinline__ int trie_child(const emu_token_trie& t, int node, int id) {
    int lo, hi;
    if (!trie_edges(t, node, lo, hi)) return -1;
    const int e = trie_lower_bound(t.tok, lo, hi, id);
    if (e >= hi || t.tok[e] != id) return -1;
    const int c = t.child[e];
    return c >= 0 && c < t.nodes ? c : -1;
}

}  // namespace

// the host-side refusals shared by the constrained entry points
static inline bool trie_args_ok(const emu_token_trie* t, const int32_t* node) {
    return t && node && t->first && t->nodes >= 1 && t->edges >= 0 && (t->edges == 0 || (t->tok && t->child));
}
