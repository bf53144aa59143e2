// Few-row (4..16) weight stream over the 13-bit lossless bf16 format (bf16_pack.h): the packed twin of thin_stream_kernel
// (gemv_thin.hip) at kch = 32:  out[m, n] = epilogue( sum_k x[m, k] * W[n, k] ), the weights from the planes of an existing
// PackSet (R = 2 or 4 rows per group: the sets of the one-row streams, gemv_pack.hip), 13/16 of the bf16 stream's HBM bytes.
//
// A workgroup (4 waves) owns RN = 16 / 32 weight rows and walks K in stages of 256.  A stage of a row group is contiguous in every
// plane, so the stage image -- low bytes RN * 256 B, nibbles RN * 128 B, signs RN * 32 B, then the MR = 8 / 16 activation rows -- is
// moved by LDS-DMA (16 bytes per lane, one instruction = 1 KiB of the image, no VGPRs): the planes non-temporal, the activations
// cached, NSTG stages deep, counted vmcnt + one raw s_barrier per stage, as the siblings do.  The image is RN / 4 + RN / 8 + 1 weight
// instructions (RN = 32: 13; RN = 16: 7, the sign instruction's upper 32 lanes repeat the lower ones into 512 bytes nothing reads)
// and MR / 2 activation instructions: 17 / 21 / 11 / 15, no multiple of the four waves.  Wave w issues instructions w, w + 4, ..
// below the total, and waits on ITS OWN compile-time vmcnt count (the branch on the wave index is scalar): nothing is padded.
//
// Lane (i, g) of wave w builds the A fragment of weight row i of a 16-row block, 16-byte k chunk c = (2 w + s) * 4 + g, from that
// row's 8 low bytes (ds_read_b64), its nibble dword (ds_read_b32) and its share of the group's sign bytes (R = 4: the group's dword,
// R = 2: the group's 16 bits) with pack_decode_row (bf16_pack.h).  B fragments, the MFMA, which k-steps a wave multiplies and in
// which order over the stages, the four-way LDS reduction and the epilogue are thin_stream.h's at kch = 32 (thin_stream_finish is
// called as it is), so the outputs are the bf16 stream's bit for bit; RN, MR and the ring depth do not enter the sum.
//
// LDS placement.  Which 16 bytes a lane's DMA fetches is free, so every plane piece is stored with its 16-byte slots XOR-swizzled
// such that the reads of a 32-lane half (16 rows x 2 adjacent chunks, the banking group of ds_read_b64 / _b32 / _u16) touch every
// bank once (low bytes: 8 row pairs x 2 chunks = 16 slots = the 64 banks; nibbles: 32 dwords = the 32 banks) or at most once
// (signs: 8 dwords; lanes that share a dword broadcast): conflict-free throughout.  The activation rows keep the bf16 kernel's
// slot ^ (row & 15).
//
// Flags.  The flag word of the workgroup's groups (RN / R <= 16 of them, aligned: one word) is requested first, the first NSTG - 1
// packed stages behind it; a workgroup with a flagged group then drains them and streams the bf16 rows through thin_stream_loop
// itself, three stages deep where three bf16 images ((RN + MR) * 512 bytes each) fit the packed ring, else two; the ring is sized for
// the larger of the two.  The branch is workgroup-uniform; no workgroup waits for another.
// Ragged N: row pairs / groups past the set's last are clamped to the last (the sets are padded to whole groups, so no load leaves
// a plane); rows >= N and columns >= M fail the epilogue's tests.  Vector stores only, no atomics: results repeat bit for bit.
//
// The plane pieces are read with ds_read instructions written out (one lgkmcnt wait for all of a stage's): the compiler guards a
// plain 8- / 4- / 2-byte LDS load behind pending LDS-DMA with s_waitcnt vmcnt(0), which emptied the ring every stage (1.25-1.5 x the
// bf16 stream's time; with it gone 0.82-0.99, profiles/bf16_pack_wide.md).
//
// hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950, the three epilogues alike but for 8 SGPRs; no scratch anywhere:
//   R  RN  MR  NSTG   VGPRs  AGPRs  SGPRs   LDS bytes  workgroups / CU (LDS)
//   4  16   8    4      39      4   45-53      45056    3
//   4  16   8    6      40      4   45-53      67584    2
//   4  16  16    3      42      4   45-53      46080    3
//   4  16  16    5      42      4   45-53      76800    2
//   4  32   8    3      64     12   54-62      52224    3
//   4  32   8    4      58      8   54-62      69632    2
//   4  32  16    3      66     12   54-62      64512    2
//   2  ..: the same LDS; VGPRs 40, 40, 42, 42, 61, 59, 63
#include "common.h"
#include "kernels.h"
#include "gemm_tile.h"
#include "bf16_pack.h"
#include "thin_stream.h"

using namespace emu_gemm;
using namespace emu_thin;

namespace {

template <int RN, int MR>
struct PackImage {                      // one stage in LDS, in 1-KiB DMA instructions and bytes
    static constexpr int NLO = RN / 4, NNIB = RN / 8, NW = NLO + NNIB + 1, TOT = NW + MR / 2;
    static constexpr int LO = 0, NIB = NLO * 1024, SIGN = (NLO + NNIB) * 1024, ACT = NW * 1024, BYTES = TOT * 1024;
};

template <int EPI, int R, int RN, int MR, int NSTG>
__global__ __launch_bounds__(256) void pack_thin_kernel(const GemvArgs a, const PackSet p, const int groups) {
    using IM = PackImage<RN, MR>;
    constexpr int RG = RN / 16, KSW = 2;                                      // kch = 32: two k-steps per wave and stage
    constexpr int NSTG_B = 3 * (RN + MR) * 512 <= NSTG * IM::BYTES ? 3 : 2;   // the flagged branch's ring: three stages where they fit the packed ring
    constexpr int TOT = IM::TOT, LPT = (TOT + 3) / 4, XTRA = TOT % 4;         // waves [0, XTRA) issue LPT instructions, the others LPT - 1
    constexpr int RING = NSTG * IM::BYTES, RING_B = thin_ring_bytes<RN, MR, NSTG_B, 32>(), RED = thin_red_bytes<RN>();
    static_assert(RN == 16 || RN == 32, "built for 16 and 32 weight rows");
    static_assert((NSTG - 2) * LPT <= 63, "vmcnt field is 6 bits");
    __shared__ __attribute__((aligned(16))) char smem[RING > RING_B ? (RING > RED ? RING : RED) : (RING_B > RED ? RING_B : RED)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * RN;
    const int g0 = n0 / R;                                                    // first row group; RN / R of them, inside one flag word
    const uint32_t fw = p.flags[g0 >> 5];                                     // requested first, used behind the prologue's DMA
    const int KV = a.K >> 3, nk = a.K >> 8;

    // DMA sources: instruction q = j * 4 + wave writes bytes [q * 1024, q * 1024 + 1024) of the image, lane l its slot l
    const char* src[LPT];
    int step[LPT];                                                            // bytes per stage of the plane the instruction reads
#pragma unroll
    for (int j = 0; j < LPT; ++j) {
        const int q = j * 4 + wave;
        const char* s0;
        int st;
        if (q < IM::NLO) {                                                    // low bytes: row pair u = row / 2, 32 slots (the stage's vi)
            const int u = 2 * q + (lane >> 5), pslot = lane & 31;
            const int units = groups * (R / 2);
            const int U = n0 / 2 + u < units ? n0 / 2 + u : units - 1;
            s0 = reinterpret_cast<const char*>(p.lo) + ((size_t)U * KV + (pslot ^ (2 * (u & 7)))) * 16;
            st = 512;
        } else if (q < IM::NLO + IM::NNIB) {
            const int qq = q - IM::NLO;
            if constexpr (R == 4) {                                           // nibbles: group gg, 32 slots of 4 row dwords
                const int gg = 2 * qq + (lane >> 5), pslot = lane & 31;
                const int G = g0 + gg < groups ? g0 + gg : groups - 1;
                s0 = reinterpret_cast<const char*>(p.nib) + ((size_t)G * KV + (pslot ^ (2 * (gg & 3)))) * 16;
                st = 512;
            } else {                                                          // 16 slots of two vi x 2 row dwords
                const int gg = 4 * qq + (lane >> 4), pslot = lane & 15;
                const int G = g0 + gg < groups ? g0 + gg : groups - 1;
                s0 = reinterpret_cast<const char*>(p.nib) + (size_t)G * KV * 8 + (pslot ^ (gg & 7)) * 16;
                st = 256;
            }
        } else if (q < IM::NW) {
            if constexpr (R == 4) {                                           // signs: group gg, 8 slots of 4 vi x one dword
                const int gg = (lane >> 3) % (RN / 4), pslot = lane & 7;
                const int G = g0 + gg < groups ? g0 + gg : groups - 1;
                s0 = reinterpret_cast<const char*>(p.sign) + (size_t)G * KV * 4 + (pslot ^ (gg & 3)) * 16;
                st = 128;
            } else {                                                          // 4 slots of 8 vi x 2 row bytes
                const int gg = (lane >> 2) % (RN / 2), pslot = lane & 3;
                const int G = g0 + gg < groups ? g0 + gg : groups - 1;
                s0 = reinterpret_cast<const char*>(p.sign) + (size_t)G * KV * 2 + (pslot ^ ((gg >> 1) & 3)) * 16;
                st = 64;
            }
        } else {                                                              // activation row r (clamped at M - 1), slot ^ (r & 15)
            const int r = 2 * (q - IM::NW) + (lane >> 5), pslot = lane & 31;
            const int m = r < a.M ? r : a.M - 1;
            s0 = reinterpret_cast<const char*>(a.x + (size_t)m * a.ldx) + (pslot ^ (r & 15)) * 16;
            st = 512;
        }
        src[j] = s0; step[j] = st;
    }
    auto issue = [&](int kt, int stage) {
        kt = kt < nk ? kt : nk - 1;                    // past-the-end stages re-load the last one (the per-wave counts stay fixed)
        char* base = smem + stage * IM::BYTES + wave * 1024;
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            const int q = j * 4 + wave;
            const char* from = src[j] + (size_t)kt * step[j];
            if (j * 4 + 3 < IM::NW) glds16_nt(from, base + j * 4096);                               // every wave: a plane, streamed
            else if (j * 4 >= IM::NW && j * 4 + 3 < TOT) glds16(from, base + j * 4096);            // every wave: activations
            else if (q < IM::NW) glds16_nt(from, base + j * 4096);
            else if (q < TOT) glds16(from, base + j * 4096);
        }
    };
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t) issue(t, t);

    const int ng = groups - g0 < RN / R ? groups - g0 : RN / R;               // the workgroup's groups that exist
    const bool flagged = __builtin_amdgcn_readfirstlane((fw >> (g0 & 31)) & ((1u << ng) - 1u)) != 0u;
    f32x4_t acc[RG];
    if (flagged) {                                     // workgroup-uniform: the bf16 rows through the bf16 stream's own loop
        wait_vmcnt<0>();
        __syncthreads();
        thin_stream_loop<RN, MR, NSTG_B, 32>(a, smem, n0, acc);
    } else {
        // this lane's reads of a stage image: weight row nl = 16 rg + i, chunk c[s]; activation row min(i, M - 1)
        int olo[KSW][RG], onib[KSW][RG], osg[KSW][RG], oact[KSW];
        const int rb = i < a.M ? i : a.M - 1;
#pragma unroll
        for (int s = 0; s < KSW; ++s) {
            const int c = (KSW * wave + s) * 4 + g;
            oact[s] = IM::ACT + rb * 512 + ((c ^ (rb & 15)) << 4);
#pragma unroll
            for (int rg = 0; rg < RG; ++rg) {
                const int nl = rg * 16 + i, u = nl >> 1;
                olo[s][rg] = IM::LO + u * 512 + ((c ^ (2 * (u & 7))) << 4) + 8 * (nl & 1);
                if constexpr (R == 4) {
                    const int gg = nl >> 2;
                    onib[s][rg] = IM::NIB + gg * 512 + ((c ^ (2 * (gg & 3))) << 4) + 4 * (nl & 3);
                    osg[s][rg] = IM::SIGN + gg * 128 + (((c >> 2) ^ (gg & 3)) << 4) + 4 * (c & 3);
                } else {
                    const int gg = nl >> 1;
                    onib[s][rg] = IM::NIB + gg * 256 + (((c >> 1) ^ (gg & 7)) << 4) + 8 * (c & 1) + 4 * (nl & 1);
                    osg[s][rg] = IM::SIGN + gg * 64 + (((c >> 3) ^ ((gg >> 1) & 3)) << 4) + 2 * (c & 7);
                }
            }
        }
        const uint32_t hb4 = (uint32_t)p.hb * 0x01010101u;
        // The plane pieces are read by ds_read instructions written out: the compiler guards a plain 8- / 4- / 2-byte LDS load behind
        // pending LDS-DMA with s_waitcnt vmcnt(0), which would end the ring's overlap (the 16-byte fragment loads are not guarded)
        const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
#pragma unroll
        for (int rg = 0; rg < RG; ++rg) acc[rg] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt < nk; ++kt) {
            if (XTRA == 0 || wave < XTRA) wait_vmcnt<(NSTG - 2) * LPT>();     // this wave's share of stage kt has landed
            else wait_vmcnt<(NSTG - 2) * (LPT - 1)>();
            __builtin_amdgcn_s_barrier();              // ... and everyone's; everyone is done reading stage kt - 1
            issue(kt + NSTG - 1, (kt + NSTG - 1) % NSTG);
            const char* sb = smem + (kt % NSTG) * IM::BYTES;
            const uint32_t sbo = lds0 + (kt % NSTG) * IM::BYTES;
            bf16x8_t bf[KSW], af[KSW][RG];
            uint64_t L[KSW][RG];
            uint32_t nb[KSW][RG], S[KSW][RG];
#pragma unroll
            for (int s = 0; s < KSW; ++s) {
                bf[s] = *reinterpret_cast<const bf16x8_t*>(sb + oact[s]);
#pragma unroll
                for (int rg = 0; rg < RG; ++rg) {
                    if constexpr (R == 4)
                        asm volatile("ds_read_b64 %0, %3\n\tds_read_b32 %1, %4\n\tds_read_b32 %2, %5"
                                     : "=&v"(L[s][rg]), "=&v"(nb[s][rg]), "=&v"(S[s][rg])
                                     : "v"(sbo + olo[s][rg]), "v"(sbo + onib[s][rg]), "v"(sbo + osg[s][rg]) : "memory");
                    else
                        asm volatile("ds_read_b64 %0, %3\n\tds_read_b32 %1, %4\n\tds_read_u16 %2, %5"
                                     : "=&v"(L[s][rg]), "=&v"(nb[s][rg]), "=&v"(S[s][rg])
                                     : "v"(sbo + olo[s][rg]), "v"(sbo + onib[s][rg]), "v"(sbo + osg[s][rg]) : "memory");
                }
            }
#pragma unroll
            for (int s = 0; s < KSW; ++s)
#pragma unroll
                for (int rg = 0; rg < RG; ++rg) {
                    if (s == 0 && rg == 0)             // one wait for all of them (LDS returns in order), tied to every value it guards
                        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(L[0][0]), "+v"(nb[0][0]), "+v"(S[0][0]), "+v"(L[KSW - 1][RG - 1]),
                                     "+v"(nb[KSW - 1][RG - 1]), "+v"(S[KSW - 1][RG - 1]) :: "memory");
                    uint32_t w[4];
                    pack_decode_row<R>((uint32_t)L[s][rg], (uint32_t)(L[s][rg] >> 32), nb[s][rg], S[s][rg], i & (R - 1), hb4, w);
                    af[s][rg] = __builtin_bit_cast(bf16x8_t, u32x4{w[0], w[1], w[2], w[3]});
                }
#pragma unroll
            for (int s = 0; s < KSW; ++s)
#pragma unroll
                for (int rg = 0; rg < RG; ++rg)
                    acc[rg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s][rg], bf[s], acc[rg], 0, 0, 0);
        }
        wait_vmcnt<0>();                               // drain the tail DMA before the ring is reused
        __syncthreads();
    }
    thin_stream_finish<EPI, RN>(a, smem, n0, acc);
}

template <int R, int RN, int MR, int NSTG>
int launch_pack_thin(const GemvArgs& a, const PackSet& p, const GemvPlan& pl, hipStream_t s) {
    const int groups = (int)pack_groups(a.N, R);
#define EMU_PT_CASE(E) case E: hipLaunchKernelGGL((pack_thin_kernel<E, R, RN, MR, NSTG>), dim3(pl.grid), dim3(pl.block), 0, s, a, p, groups); break;
    switch (a.epi) {
        EMU_PT_CASE(EPI_NONE) EMU_PT_CASE(EPI_RESID) EMU_PT_CASE(EPI_SWIGLU)
        default: return -22;
    }
#undef EMU_PT_CASE
    EMU_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// the built (set rows, weight rows, activation rows, ring depth) combinations; gemv.hip::gemv_pack_thin_plan picks among them.  What
// only pointers can answer is checked here: the set's four pointers, 16-byte aligned planes (the DMA's unit), x, W, out, res.
int launch_gemv_pack_thin(const GemvArgs& a, const PackSet& p, const GemvPlan& pl, hipStream_t s) {
    if (pl.status || pl.family != GEMV_FAM_PACK_THIN || pl.kch != 32 || pl.block != 256) return -22;
    if (!a.x || !a.W || !a.out || !p.lo || !p.nib || !p.sign || !p.flags || (a.epi == EPI_RESID && !a.res)) return -22;
    if ((reinterpret_cast<size_t>(p.lo) | reinterpret_cast<size_t>(p.nib) | reinterpret_cast<size_t>(p.sign) | reinterpret_cast<size_t>(a.x) |
         reinterpret_cast<size_t>(a.W)) & 15) return -22;
    if (a.M < 4 || a.M > pl.mb || a.K < 256 || (a.K & 255) || a.ldw < a.K || (a.ldw & 7) || (a.ldx & 7) || p.hb < 0 || p.hb > 112) return -22;
    if (pl.grid != (a.N + pl.rows - 1) / pl.rows) return -22;
    constexpr auto key = [](int set_rows, int rows, int mb, int stages) { return ((set_rows * 100 + rows) * 100 + mb) * 10 + stages; };
    switch (key(p.rows, pl.rows, pl.mb, pl.stages)) {
        case key(4, 32, 8, 4): return launch_pack_thin<4, 32, 8, 4>(a, p, pl, s);
        case key(4, 32, 8, 3): return launch_pack_thin<4, 32, 8, 3>(a, p, pl, s);
        case key(4, 32, 16, 3): return launch_pack_thin<4, 32, 16, 3>(a, p, pl, s);
        case key(4, 16, 8, 4): return launch_pack_thin<4, 16, 8, 4>(a, p, pl, s);
        case key(4, 16, 8, 6): return launch_pack_thin<4, 16, 8, 6>(a, p, pl, s);
        case key(4, 16, 16, 5): return launch_pack_thin<4, 16, 16, 5>(a, p, pl, s);
        case key(4, 16, 16, 3): return launch_pack_thin<4, 16, 16, 3>(a, p, pl, s);
        case key(2, 32, 8, 4): return launch_pack_thin<2, 32, 8, 4>(a, p, pl, s);
        case key(2, 32, 8, 3): return launch_pack_thin<2, 32, 8, 3>(a, p, pl, s);
        case key(2, 32, 16, 3): return launch_pack_thin<2, 32, 16, 3>(a, p, pl, s);
        case key(2, 16, 8, 4): return launch_pack_thin<2, 16, 8, 4>(a, p, pl, s);
        case key(2, 16, 8, 6): return launch_pack_thin<2, 16, 8, 6>(a, p, pl, s);
        case key(2, 16, 16, 5): return launch_pack_thin<2, 16, 16, 5>(a, p, pl, s);
        case key(2, 16, 16, 3): return launch_pack_thin<2, 16, 16, 3>(a, p, pl, s);
        default: return -22;
    }
}
