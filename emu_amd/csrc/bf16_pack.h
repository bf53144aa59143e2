// The 13-bit and 12-bit lossless bf16 weight formats of the one-row decode streams (the 12-bit one below the 13-bit one): the ONE place that states the layout, shared by the packer
// (bf16_pack.hip) and the stream kernels (gemv_pack.hip; gemv_pack_thin.hip at 4..16 rows, both formats); emu_amd/bf16pack.py restates it with torch on the CPU.
//
// A weight matrix uses a handful of binades, so the top 7 bits of a bf16's exponent field fit a 4-bit offset from a per-matrix
// base hb.  A weight w (16 bits: s, e8, m7) is kept as three pieces:
//     low byte   w & 0xff                      (e8's lowest bit and the mantissa), verbatim
//     nibble     ((w >> 8) & 0x7f) - hb        in 0..15
//     sign       w >> 15
// hb comes from the largest exponent field emax of the finite weights: top = emax | 1, hb = max(0, (top - 31) >> 1): the window is the
// 32 binades [2 hb, 2 hb + 31].  A weight outside it (a zero or a tiny value next to large ones, Inf / NaN) flags its row group in a
// per-matrix bitmap; a flagged workgroup streams the bf16 rows instead (workgroup-uniform), so nothing is patched in the stream.
//
// Layout.  Which weights a thread owns is the partition of the bf16 kernel the planner picks for the shape (thread t of the 256 owns
// the 16-byte vectors t, t + 256, ... of each of the R rows of its workgroup, emu_gemv_partition == 4), so the planes are laid out per
// row group g (R = 2 or 4 consecutive rows, the last group padded with zero weights) and vector index vi (8 weights of each row),
// KV = K / 8, every load of a wave contiguous:
//     low plane    16-byte unit (g, h, vi) at ((g * R/2 + h) * KV + vi) * 16, h < R/2: rows 2h and 2h + 1 of the group, per row the
//                  dwords L0 (low bytes of weights 0..3, weight j in byte j) and L1 (weights 4..7)
//     nibbles      R dwords at (g * KV + vi) * 4 R: dword r, byte b = nibble of weight b | nibble of weight b + 4 << 4 of row r
//     signs        R bytes at (g * KV + vi) * R.  R = 2: byte r, bit j = sign of weight j of row r.  R = 4: the four bytes are one
//                  32-bit word whose bit 8 b + 7 - q holds the sign of weight 4 hf + b of row r, q = 2 r + hf: the signs of four
//                  weights that share a dword of high bytes sit one byte apart, so (word << q) & 0x80808080 is their mask
//     flags        one bit per row group, 32-bit words
// That is 13 bits per weight: 16-byte loads for the low and (R = 4) nibble planes, 4-byte (R = 4) / 2-byte (R = 2) loads for the signs.
#pragma once
#include <stdint.h>

struct PackSet {                    // one matrix's packed set as the kernels take it
    const void* lo = nullptr;
    const void* nib = nullptr;
    const void* sign = nullptr;
    const uint32_t* flags = nullptr;
    int hb = 0;                     // the matrix's exponent base
    int rows = 0;                   // R: rows per group (the rows per workgroup of the planned form), 0 = no set
    const uint32_t* patch = nullptr;   // the 12-bit format below: its patch records (sign is null then); null = the 13-bit format
};

constexpr int pack_hb(int emax) { return (emax | 1) < 31 ? 0 : ((emax | 1) - 31) >> 1; }       // (constexpr: host and device)
constexpr size_t pack_groups(int N, int R) { return ((size_t)N + R - 1) / R; }
inline size_t pack_lo_bytes(int N, int K, int R) { return pack_groups(N, R) * (size_t)R * K; }
inline size_t pack_nib_bytes(int N, int K, int R) { return pack_groups(N, R) * (size_t)R * K / 2; }
inline size_t pack_sign_bytes(int N, int K, int R) { return pack_groups(N, R) * (size_t)R * K / 8; }
inline size_t pack_flag_words(int N, int R) { return (pack_groups(N, R) + 31) / 32; }


// ---- The 12-bit format: the same low plane, and the sign moves into the nibble, so the sign plane goes.  A matrix's weights sit in far
// fewer than 32 binades, so a window of 8 exponent-pair codes (16 binades) from a per-matrix base hb holds all but a few tiny ones:
//     nibble     n(w) = (w >> 15) << 3 | code,  code = ((w >> 8) & 0x7f) - hb  in 0..7
// laid out as the 13-bit nibbles are (byte b of row r = n(w_b) | n(w_{b+4}) << 4).  A weight whose code is outside 0..7 -- any bit
// pattern: zeros, denormals, Inf and NaN are not special -- is a miss: its low byte stays in the low plane, its nibble is 0 and one
// slot of the row group's patch record carries its true high byte:
//     patch      8 slots of 32 bits per row group at patch + g * 32 bytes.  slot = vi << 13 | r << 11 | j << 8 | (w >> 8): vector index
//                vi (bits 13..31: the owning lane vi & 255 at bits 13..20, its trip vi >> 8 at bits 21..31), row r in the group, element
//                j of the vector, high byte.  An empty slot is 0xffffffff, whose trip 2047 no kernel runs (KV <= 2304).  The slots in
//                use are sorted ascending (by vi, r, j), the empty ones behind them.
//     flags      a group with more than 8 misses is flagged, streams its bf16 rows as in the 13-bit format, and its record is empty
// Rows that pad the last group are no misses (nibble 0, low byte 0).  hb is the base of the 8-code window that covers the most weights,
// from the 128-bin histogram of (w >> 8) & 0x7f over the matrix; ties go to the lower base (pack12_window; bf16pack.py: window_rule).
// 12 bits per weight in two planes: one load instruction fewer per trip than the 13-bit set.
constexpr int PACK12_SLOTS = 8;
constexpr uint32_t PACK12_EMPTY = 0xffffffffu;
constexpr int PACK12_MAX_KV = 1 << 18;             // vi must stay clear of the empty slot's
inline size_t pack12_patch_bytes(int N, int R) { return pack_groups(N, R) * PACK12_SLOTS * 4; }
constexpr uint32_t pack12_slot(uint32_t vi, int r, int j, uint32_t high) { return vi << 13 | (uint32_t)r << 11 | (uint32_t)j << 8 | high; }
inline int pack12_window(const unsigned long long (&hist)[128]) {
    unsigned long long best = 0, cur = 0;
    int hb = 0;
    for (int b = 0; b < 8; ++b) cur += hist[b];
    best = cur;
    for (int b = 1; b <= 120; ++b) {
        cur += hist[b + 7] - hist[b - 1];
        if (cur > best) { best = cur; hb = b; }
    }
    return hb;
}

#ifdef __HIPCC__
// the pieces of 8 weights of row r of a group of R (the dwords w.x .. w.w of a 16-byte bf16 vector): low bytes L0 / L1, nibble
// dword, and the row's share of the group's sign bytes (R = 2: its byte at bits 8 r; R = 4: its bits of the word);
// bad: some weight's nibble is outside 0..15 or its exponent field is 255
template <int R>
__device__ __forceinline__ void pack_encode_row(const uint32_t (&w)[4], int r, int hb, uint32_t& L0, uint32_t& L1, uint32_t& nib, uint32_t& sign,
                                                bool& bad) {
    L0 = L1 = nib = sign = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t v = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        const int d = (int)((v >> 8) & 0x7f) - hb;
        bad = bad || d < 0 || d > 15 || ((v >> 7) & 0xff) == 0xff;
        if (j < 4) L0 |= (v & 0xff) << (8 * j); else L1 |= (v & 0xff) << (8 * (j - 4));
        nib |= (uint32_t)(d & 15) << (8 * (j & 3) + 4 * (j >> 2));
        sign |= (v >> 15) << (R == 4 ? 8 * (j & 3) + 7 - (2 * r + (j >> 2)) : 8 * r + j);
    }
}

// a * b on the full-rate 24-bit multiplier (the compiler picks the quarter-rate v_mul_lo_u32 for the same product)
__device__ __forceinline__ uint32_t pack_mul24(uint32_t a, uint32_t b) {
    uint32_t d;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
// 8 weights of row r of a group of R back to the four bf16-pair dwords of their 16-byte vector, four weights at a time: the high
// bytes are H = (nibbles as bytes + hb in every byte) | signs at bit 7 of every byte, and two v_perm_b32 interleave H with the low
// bytes.  The signs: R = 4, one shift of the group's word S; R = 2, the 24-bit multiply of four sign bits by 0x204081 puts bit i at
// bit 8 i (no two partial products meet, so nothing carries).  hb4 = hb * 0x01010101.
template <int R>
__device__ __forceinline__ void pack_decode_row(uint32_t L0, uint32_t L1, uint32_t nib, uint32_t S, int r, uint32_t hb4, uint32_t (&w)[4]) {
    uint32_t ha = (nib & 0x0f0f0f0fu) + hb4;
    uint32_t hh = ((nib >> 4) & 0x0f0f0f0fu) + hb4;
    if constexpr (R == 4) {
        ha |= (S << (2 * r)) & 0x80808080u;
        hh |= (S << (2 * r + 1)) & 0x80808080u;
    } else {
        ha |= (pack_mul24(__builtin_amdgcn_ubfe(S, 8 * r, 4), 0x204081u) << 7) & 0x80808080u;
        hh |= (pack_mul24(__builtin_amdgcn_ubfe(S, 8 * r + 4, 4), 0x204081u) << 7) & 0x80808080u;
    }
    w[0] = __builtin_amdgcn_perm(ha, L0, 0x05010400u);
    w[1] = __builtin_amdgcn_perm(ha, L0, 0x07030602u);
    w[2] = __builtin_amdgcn_perm(hh, L1, 0x05010400u);
    w[3] = __builtin_amdgcn_perm(hh, L1, 0x07030602u);
}

// ---- the 12-bit format.  Encode: the low bytes and the nibble dword of 8 weights; miss: bit j = weight j is a miss (its nibble 0)
__device__ __forceinline__ void pack12_encode_row(const uint32_t (&w)[4], int hb, uint32_t& L0, uint32_t& L1, uint32_t& nib, uint32_t& miss) {
    L0 = L1 = nib = miss = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t v = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        const int d = (int)((v >> 8) & 0x7f) - hb;
        const bool out = d < 0 || d > 7;
        if (j < 4) L0 |= (v & 0xff) << (8 * j); else L1 |= (v & 0xff) << (8 * (j - 4));
        if (out) miss |= 1u << j;
        else nib |= ((v >> 15) << 3 | (uint32_t)d) << (8 * (j & 3) + 4 * (j >> 2));
    }
}
// Decode: the codes as bytes + hb in every byte, the sign from bit 3 / bit 7 of each nibble pair to bit 7, then pack_decode_row's perms
__device__ __forceinline__ void pack12_decode_row(uint32_t L0, uint32_t L1, uint32_t nib, uint32_t hb4, uint32_t (&w)[4]) {
    const uint32_t ha = ((nib & 0x07070707u) + hb4) | ((nib << 4) & 0x80808080u);
    const uint32_t hh = (((nib >> 4) & 0x07070707u) + hb4) | (nib & 0x80808080u);
    w[0] = __builtin_amdgcn_perm(ha, L0, 0x05010400u);
    w[1] = __builtin_amdgcn_perm(ha, L0, 0x07030602u);
    w[2] = __builtin_amdgcn_perm(hh, L1, 0x05010400u);
    w[3] = __builtin_amdgcn_perm(hh, L1, 0x07030602u);
}
// A row group's patch record in a wave: lane s < 8 holds slot s, and key = the slot's trip and row pair (slot >> 12 with the lane field
// cleared; no slot's in the lanes from 8 up).  Rows are patched two at a time (the pair h = rows 2h and 2h + 1 of the group): the
// test "does a slot name trip `trip` and pair h" is workgroup-uniform, one v_cmp of key against a constant and a branch on vcc
struct Pack12Rec { uint32_t slot, key; };
__device__ __forceinline__ Pack12Rec pack12_record(const uint32_t* patch, int g, int lane) {
    Pack12Rec rec;
    rec.slot = patch[(size_t)g * PACK12_SLOTS + (lane & (PACK12_SLOTS - 1))];
    rec.key = lane < PACK12_SLOTS ? (rec.slot >> 12) & ~0x1feu : PACK12_EMPTY;
    return rec;
}
// the decoded dwords w[i] of the 8 weights thread tid holds of rows 2h + i of the group in trip `trip` (vi = tid + 256 trip), patched:
// skipped on the uniform test where no slot names them; else, slot by slot of those that do, the owning lane replaces the high byte
// of dword j >> 1, half j & 1 of its row (a uniform switch over the eight dwords: no indexed registers).  The ballot sees active lanes
// only and the record is in lanes 0..7: call with the whole wave, never under a per-lane `vi < KV` (a ragged trip's last wave may
// hold 4 vectors); a lane past the row matches no slot, so nothing else needs masking.
__device__ __forceinline__ void pack12_patch(const Pack12Rec& rec, int trip, int h, int tid, uint32_t (&w)[2][4]) {
    unsigned long long hit = __builtin_amdgcn_ballot_w64(rec.key == ((uint32_t)trip << 9 | (uint32_t)h));
#pragma nounroll
    while (hit) {
        const uint32_t p = __builtin_amdgcn_readlane(rec.slot, __builtin_ctzll(hit));
        hit &= hit - 1;
        const uint32_t sh = (p & 0x100u) ? 24u : 8u;
        const uint32_t m = ((p >> 13) & 255u) == (uint32_t)tid ? 0xffu << sh : 0u, high = (p & 0xffu) << sh;
        const uint32_t at = (p >> 9) & 7u;                            // 4 (r & 1) + (j >> 1)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int d = 0; d < 4; ++d)
                if (at == (uint32_t)(4 * i + d)) w[i][d] = (w[i][d] & ~m) | (high & m);
    }
}
#endif
