// Device code shared by the two MXFP4 matrix-core kernels (gemv_fp4_thin.hip: 1..16 rows, k-split units; gemm_fp4.hip: 17 rows
// and more, a two-dimensional tile): the geometry of one K stage in LDS, its two swizzles -- each defined ONCE and called by the
// DMA-source side (w_src / x_src) and by the LDS-read side (w_off / x_off), which must agree or the MFMA multiplies the wrong k --,
// the partial last stage of a K that is no multiple of 256 (source clamp and read mask), the 4-bit -> bf16 fragment conversion and
// the lane epilogue (store_c4).  glds16_nt lives in gemm_tile.h next to glds16: the bf16
// few-row stream (gemv_thin.hip) uses it too.
//
// A stage is KC = 256 k: per weight row 128 element bytes (8 MX blocks of 16 bytes) + 8 scale bytes, per activation row 512 bytes
// (32 chunks of 16 bytes).  Both arrive by 16-byte LDS-DMA, the LDS image lane-linear, the swizzle carried by the source address:
//   * weight rows are 128 bytes, so rows r and r + 2 share banks: block b of row r sits in slot b ^ ((r >> 1) & 7), which makes
//     the ds_read_b128 of 16 rows x one block conflict-free in every lane group;
//   * chunk c of activation row r sits in slot c ^ xswz(r), xswz = the two 2-bit halves of r (within its 16-row tile) swapped:
//     lanes g and g + 1 of one lane group read chunks 4 apart, which the plain c ^ r of gemv_thin.hip would fold onto the same banks.
#pragma once
#include "common.h"
#include "kernels.h"
#include "gemm_tile.h"

namespace emu_gemm {

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

constexpr int KC = 256, WROW = KC / 2, XROW = KC * 2, SROW = KC / 32;   // k per stage; bytes per staged weight / activation / scale row

// 4-byte LDS-DMA (the scale bytes).  NT: a use-once stream (aux 2), as glds16_nt; otherwise the plain form, as glds16
template <bool NT>
__device__ __forceinline__ void glds4(const void* src, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, NT ? 2 : 0);
}

// the two swizzles (an XOR: slot -> block / chunk and back are the same function)
__device__ __forceinline__ int wswz(int r) { return (r >> 1) & 7; }
__device__ __forceinline__ int xswz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

// DMA sources of a lane.  Weight instruction q of a tile at weight row n0 fills tile rows 8q .. 8q + 7 (lane / 8 selects; slot
// lane % 8 receives block w_src_blk = slot ^ wswz(row); rows clamped at N - 1).  An activation instruction fills two tile rows
// (x_dma_row: instruction qa, lane / 32 selects; slot lane % 32 receives chunk x_src_chunk = slot ^ xswz(row); rows clamped at M - 1).
__device__ __forceinline__ int w_src_blk(int q, int lane) { return (lane & 7) ^ wswz(8 * q + (lane >> 3)); }
__device__ __forceinline__ const char* w_src(const GemvArgs& a, int n0, int q, int lane) {
    const int r = 8 * q + (lane >> 3), c = w_src_blk(q, lane), n = n0 + r;
    return reinterpret_cast<const char*>(a.W) + (size_t)(n < a.N ? n : a.N - 1) * a.ldw + c * 16;
}
__device__ __forceinline__ int x_dma_row(int qa, int lane) { return 2 * qa + (lane >> 5); }
__device__ __forceinline__ int x_src_chunk(int r, int lane) { return (lane & 31) ^ xswz(r); }
__device__ __forceinline__ const char* x_src(const GemvArgs& a, int m0, int r, int lane) {
    const int c = x_src_chunk(r, lane), m = m0 + r;
    return reinterpret_cast<const char*>(a.x + (size_t)(m < a.M ? m : a.M - 1) * a.ldx) + c * 16;
}
// A partial last stage (K % 256 != 0) holds kb = (K % 256) / 32 valid MX blocks, kb = 1..7: a lane whose block (weights) or 16-byte
// chunk (activations: four per block) lies at or past K fetches the same block / chunk of the stage before -- the same row, in
// range because K >= 256, the same slot -- so nothing is read past a row's K, and what lands in those slots is dead: the read side
// (tail_mask_w / tail_mask_x) keeps it out of the MFMA.  *_src_past: this lane's source of instruction q / activation row r is such a one.
__device__ __forceinline__ bool w_src_past(int q, int lane, int kb) { return w_src_blk(q, lane) >= kb; }
__device__ __forceinline__ bool x_src_past(int r, int lane, int kb) { return x_src_chunk(r, lane) >= 4 * kb; }
// LDS-read side: byte offset of MX block blk in staged weight row r, and of chunk c in staged activation row r
__device__ __forceinline__ int w_off(int r, int blk) { return r * WROW + ((blk ^ wswz(r)) << 4); }
__device__ __forceinline__ int x_off(int r, int c) { return r * XROW + ((c ^ xswz(r)) << 4); }

// E8M0 scale byte -> the scale operand of the conversion: a float whose exponent field is the byte (2^(byte - 127))
__device__ __forceinline__ float scale_operand(uint32_t byte) { return __uint_as_float(byte << 23); }
// The read side of a partial last stage: block blk >= kb is dead.  Whatever its LDS slots hold (the stage before; scale padding,
// which may be 0xFF = NaN), the lane multiplies nothing: code 0 under scale 2^0 times activation 0 -- exactly the products of a
// matrix extended to the next multiple of 256 with code 0, scale byte 127 and zero activations.
__device__ __forceinline__ void tail_mask_w(bool live, u32x4& wv, float& sc) {
    if (!live) { wv = u32x4{0u, 0u, 0u, 0u}; sc = 1.f; }
}
__device__ __forceinline__ bf16x8_t tail_mask_x(bool live, bf16x8_t bf) {
    const u32x4 z = live ? __builtin_bit_cast(u32x4, bf) : u32x4{0u, 0u, 0u, 0u};
    return __builtin_bit_cast(bf16x8_t, z);
}
// one dword of element bytes (8 codes) -> the 8 bf16 of an MFMA fragment, scaled by 2^(exponent field of sc - 127)
__device__ __forceinline__ bf16x8_t cvt8(uint32_t d, float sc) {
    const bf16x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 0);
    const bf16x2_t p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 1);
    const bf16x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 2);
    const bf16x2_t p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 3);
    return bf16x8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// The epilogue of one MFMA lane: the lane holds v[r] = C[weight row nb + r][activation row m], r = 0..3, i.e. 4 consecutive output
// columns of row m < M.  Bias, round to bf16, then the residual or SiLU(gate) * up on interleaved rows: the rounding points of both
// 4-bit kernels, which are those of thin_stream_kernel (gemv_thin.hip keeps its own copy with the SiLU / GELU branches: as a shared
// function it changed that kernel's register counts, profiles/fp4_tile_refactor_equivalence.md).  8 bytes packed when the four
// columns are in range and the address is aligned, scalar stores otherwise.
template <int EPI>
__device__ __forceinline__ void store_c4(const GemvArgs& a, int m, int nb, f32x4_t v) {
    if constexpr (EPI == EPI_SWIGLU) {
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
            const int n = nb + r;
            if (n + 1 < a.N) {
                float gt = v[r], up = v[r + 1];
                if (a.bias) { gt += bf2f(a.bias[n]); up += bf2f(a.bias[n + 1]); }
                gt = bfround(gt); up = bfround(up);
                a.out[(size_t)m * a.ldo + (n >> 1)] = f2bf(bfround(silu(gt)) * up);
            }
        }
    } else {
        float o[4];
        const bool full = nb + 3 < a.N;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = nb + r;
            float t = v[r];
            if (n < a.N) {
                if (a.bias) t += bf2f(a.bias[n]);
                t = bfround(t);
                if constexpr (EPI == EPI_RESID) t = t + bf2f(a.res[(size_t)m * a.ldres + n]);
            }
            o[r] = t;
        }
        bf16_t* dst = a.out + (size_t)m * a.ldo + nb;
        if (full && ((reinterpret_cast<size_t>(dst) & 7) == 0)) {
            uint2 pk;
            pk.x = packbf(o[0], o[1]); pk.y = packbf(o[2], o[3]);
            *reinterpret_cast<uint2*>(dst) = pk;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (nb + r < a.N) dst[r] = f2bf(o[r]);
        }
    }
}

}  // namespace emu_gemm
