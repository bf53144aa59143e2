// The 13-bit lossless bf16 weight format of the one-row decode streams: the ONE place that states the layout, shared by the packer
// (bf16_pack.hip) and the stream kernels (gemv_pack.hip); emu_amd/bf16pack.py restates it with torch on the CPU.
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
};

constexpr int pack_hb(int emax) { return (emax | 1) < 31 ? 0 : ((emax | 1) - 31) >> 1; }       // (constexpr: host and device)
constexpr size_t pack_groups(int N, int R) { return ((size_t)N + R - 1) / R; }
inline size_t pack_lo_bytes(int N, int K, int R) { return pack_groups(N, R) * (size_t)R * K; }
inline size_t pack_nib_bytes(int N, int K, int R) { return pack_groups(N, R) * (size_t)R * K / 2; }
inline size_t pack_sign_bytes(int N, int K, int R) { return pack_groups(N, R) * (size_t)R * K / 8; }
inline size_t pack_flag_words(int N, int R) { return (pack_groups(N, R) + 31) / 32; }

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
#endif
