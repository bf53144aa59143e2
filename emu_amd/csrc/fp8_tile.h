// Device code shared by the two fp8 (e4m3, W8A16) matrix-core kernels (gemv_fp8_thin.hip: 1..16 rows, k split over the waves;
// gemm_fp8.hip: 17..64 rows, a two-dimensional tile, and 65 rows and more, the same tile at 128 activation rows on a two-dimensional
// grid): the geometry of one K stage in LDS and the e4m3 -> bf16 fragment conversion.
// A stage is F8_KC = 256 k: 256 bytes per weight row (16 chunks of 16 bytes), 512 per activation row (32 chunks).  Both arrive by
// 16-byte LDS-DMA, the LDS image lane-linear, the swizzle carried by the source address: chunk c of staged row r sits in slot
// c ^ (r & 15).  The epilogue (store_c4) is fp4_tile.h's.
#pragma once
#include "fp4_tile.h"

namespace emu_gemm {

constexpr int F8_KC = 256, F8_WROW = F8_KC, F8_XROW = F8_KC * 2;     // k per stage; bytes per staged weight / activation row

// two dwords of e4m3 bytes (8 codes, byte j = element j) -> the 8 bf16 of an MFMA fragment
__device__ __forceinline__ bf16x8_t cvt8_e4m3(uint32_t d0, uint32_t d1) {
    const bf16x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, false);
    const bf16x2_t p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, true);
    const bf16x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, false);
    const bf16x2_t p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, true);
    return bf16x8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

}  // namespace emu_gemm
