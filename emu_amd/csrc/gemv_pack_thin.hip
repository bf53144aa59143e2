// Few-row (4..16) weight stream over the 13-bit lossless bf16 format (bf16_pack.h; BITS = 12, below the table: the 12-bit one): the packed twin of thin_stream_kernel
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
//
// BITS = 12: the twin over the 12-bit sets (bf16_pack.h), so that the one resident set of a matrix serves its one-row stream and
// this one.  The BITS = 13 instantiations are the instructions they were (--save-temps, compared function by function).  Three things
// differ.  The stage image has no sign piece: RN / 4 + RN / 8 weight instructions (12 / 6), 1 KiB less per stage, every count above
// following from TOT.  A fragment is one ds_read_b64 and one ds_read_b32 through pack12_decode_row.  And the workgroup's RN / R row
// groups bring 8 patch slots each (at most 128 of 4 bytes): lane l of every wave loads slot l (+ 64) by a written-out
// global_load_dword beside the flag word, ahead of the prologue's DMA, and waits for it by count behind the prologue -- (NSTG - 1) x
// the fewest instructions a wave issues per stage may stay in flight, loads return in order; ONE wait statement for all waves hands
// the registers over (wait_vmcnt_records) -- so the ring is not drained (a plain load's result
// would cost vmcnt(0)).  From the slots the wave keeps, per lane, the stage of a slot that one of ITS lanes decodes (vi = 32 stage +
// 8 wave + 4 s + g) and, in two scalar registers, a bitmap of those stages built once by a scalar walk; a stage whose bit is clear
// costs that scalar test.  Otherwise a ballot finds the stage's slots and each is applied by a readlane, a lane compare and a uniform
// switch over the wave's KSW x RG x 4 decoded dwords: the high byte of half j & 1 of dword j >> 1, between the decode and the MFMA.
// The whole wave runs all of it (the ballot sees active lanes only; rows and groups past the end are clamped, and a clamped lane
// patches its clamped copy).  A flagged group still sends its workgroup through thin_stream_loop, which never looks at the records.
//   R  RN  MR  NSTG   VGPRs  AGPRs  SGPRs   LDS bytes  (12 bits; no scratch anywhere)
//   4  16   8    4      42      4   48-50      40960
//   4  16   8    6      42      4   48-50      61440
//   4  16  16    3      44      4   48-50      43008
//   4  16  16    5      44      4   48-50      71680
//   4  32   8    3      64     12   40-49      49152
//   4  32   8    4      64      8   40-49      65536
//   4  32  16    3      66     12   40-49      61440
//   2  ..: the same LDS; VGPRs 42, 42, 44, 44, 58, 58, 60; SGPRs 48-52 (16 rows), 45-53 (32 rows)
// The plan is the 13-bit twin's (gemv_pack_thin_plan): the smaller image would let some tiles take a deeper ring or one more
// workgroup per CU, which nothing has measured.
#include "common.h"
#include "kernels.h"
#include "gemm_tile.h"
#include "bf16_pack.h"
#include "thin_stream.h"

using namespace emu_gemm;
using namespace emu_thin;

namespace {

template <int RN, int MR, int BITS = 13>
struct PackImage {                      // one stage in LDS, in 1-KiB DMA instructions and bytes (12 bits: no sign piece)
    static constexpr int NLO = RN / 4, NNIB = RN / 8, NW = NLO + NNIB + (BITS == 13 ? 1 : 0), TOT = NW + MR / 2;
    static constexpr int LO = 0, NIB = NLO * 1024, SIGN = (NLO + NNIB) * 1024, ACT = NW * 1024, BYTES = TOT * 1024;
};

// s_waitcnt vmcnt(N) that hands over the patch-record registers: they are loaded by written-out instructions, so the compiler does not
// know that they are pending, and the in / out operands make every use of the records depend on this statement.  That holds only while
// it is the ONE statement through which a path passes them: with two of them under an if / else the compiler merges their outputs in a
// new register and copies the still-pending one into it AHEAD of one of the waits.  So each path has exactly one, and the ISA of every
// 12-bit instantiation has been read for it: nothing names the loads' destinations between the loads and this wait.
template <int N, int NSL>
__device__ __forceinline__ void wait_vmcnt_records(uint32_t (&v)[NSL]) {
    static_assert(NSL == 1 || NSL == 2, "one or two record registers");
    if constexpr (NSL == 1) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v[0]) : "n"(N) : "memory");
    else asm volatile("s_waitcnt vmcnt(%2)" : "+v"(v[0]), "+v"(v[1]) : "n"(N) : "memory");
}

template <int EPI, int R, int RN, int MR, int NSTG, int BITS = 13>
__global__ __launch_bounds__(256) void pack_thin_kernel(const GemvArgs a, const PackSet p, const int groups) {
    using IM = PackImage<RN, MR, BITS>;
    constexpr int RG = RN / 16, KSW = 2;                                      // kch = 32: two k-steps per wave and stage
    constexpr int NSTG_B = 3 * (RN + MR) * 512 <= NSTG * IM::BYTES ? 3 : 2;   // the flagged branch's ring: three stages where they fit the packed ring
    constexpr int TOT = IM::TOT, LPT = (TOT + 3) / 4, XTRA = TOT % 4;         // waves [0, XTRA) issue LPT instructions, the others LPT - 1
    constexpr int RING = NSTG * IM::BYTES, RING_B = thin_ring_bytes<RN, MR, NSTG_B, 32>(), RED = thin_red_bytes<RN>();
    static_assert(RN == 16 || RN == 32, "built for 16 and 32 weight rows");
    static_assert((NSTG - 2) * LPT <= 63 && (BITS == 13 || (NSTG - 1) * LPT <= 63), "vmcnt field is 6 bits");
    static_assert(BITS == 13 || BITS == 12, "the 13-bit and the 12-bit format");
    __shared__ __attribute__((aligned(16))) char smem[RING > RING_B ? (RING > RED ? RING : RED) : (RING_B > RED ? RING_B : RED)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * RN;
    const int g0 = n0 / R;                                                    // first row group; RN / R of them, inside one flag word
    const uint32_t fw = p.flags[g0 >> 5];                                     // requested first, used behind the prologue's DMA
    const int KV = a.K >> 3, nk = a.K >> 8;
    // 12 bits: the patch records of the workgroup's NG groups, 8 slots each, requested beside the flag word and ahead of every DMA:
    // lane l of EVERY wave holds slot l & 7 of group l >> 3 (+ 8 n in register n; a group past the last is clamped like its planes, so
    // its copy is patched like the original).  Written-out loads: the compiler waits vmcnt(0) at the use of a plain load's result
    // while LDS-DMA is pending; these are waited for by count behind the prologue (loads return in order)
    constexpr int NG = RN / R, NSL = BITS == 12 ? (NG * PACK12_SLOTS + 63) / 64 : 1;
    uint32_t slot[NSL];
    if constexpr (BITS == 12) {
#pragma unroll
        for (int n = 0; n < NSL; ++n) {
            const int gl = (lane >> 3) + 8 * n;
            const int G = g0 + gl < groups ? g0 + gl : groups - 1;
            const uint32_t* at = p.patch + (size_t)G * PACK12_SLOTS + (lane & (PACK12_SLOTS - 1));
            asm volatile("global_load_dword %0, %1, off" : "=v"(slot[n]) : "v"(at) : "memory");
        }
    }

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
        } else if (BITS == 13 && q < IM::NW) {
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
        if constexpr (BITS == 12) {                    // (the records' registers stay allocated until the loads have landed: read-only, no copy)
#pragma unroll
            for (int n = 0; n < NSL; ++n) asm volatile("" :: "v"(slot[n]));
        }
        __syncthreads();
        thin_stream_loop<RN, MR, NSTG_B, 32>(a, smem, n0, acc);
    } else {
        // this lane's reads of a stage image: weight row nl = 16 rg + i, chunk c[s]; activation row min(i, M - 1)
        int olo[KSW][RG], onib[KSW][RG], osg[KSW][RG], oact[KSW];              // (osg: 13 bits only)
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
                    if constexpr (BITS == 13) osg[s][rg] = IM::SIGN + gg * 128 + (((c >> 2) ^ (gg & 3)) << 4) + 4 * (c & 3);
                } else {
                    const int gg = nl >> 1;
                    onib[s][rg] = IM::NIB + gg * 256 + (((c >> 1) ^ (gg & 7)) << 4) + 8 * (c & 1) + 4 * (nl & 1);
                    if constexpr (BITS == 13) osg[s][rg] = IM::SIGN + gg * 64 + (((c >> 3) ^ ((gg >> 1) & 3)) << 4) + 2 * (c & 7);
                }
            }
        }
        const uint32_t hb4 = (uint32_t)p.hb * 0x01010101u;
        // The plane pieces are read by ds_read instructions written out: the compiler guards a plain 8- / 4- / 2-byte LDS load behind
        // pending LDS-DMA with s_waitcnt vmcnt(0), which would end the ring's overlap (the 16-byte fragment loads are not guarded)
        const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
        // 12 bits.  The weight (vi, r, j) of the workgroup's group gl is row nl = gl * R + r: it is decoded in stage vi >> 5 by wave
        // (vi & 31) >> 3, sub-step (vi >> 2) & 1, lane (i, g) = (nl & 15, vi & 3), fragment rg = nl >> 4.  key = the stage of a slot this
        // wave owns (no stage's otherwise), and bm, built once by a scalar walk over the wave's slots, has bit (stage & 127) set for
        // every such stage: a stage without a slot costs the scalar test of its bit (K > 32768: stages 128 apart share a bit, and the
        // one without a slot finds no key equal to it)
        uint32_t key[NSL];
        uint64_t bm0 = 0, bm1 = 0;
        if constexpr (BITS == 12) {
            // one statement for all four waves, so the smaller count: a wave that issues LPT - 1 instructions per stage has the records
            // behind it with the whole prologue still in flight; one that issues LPT also waits for the first NSTG - 1 of its own
            // instructions, most of which the first stage's wait below asks for anyway
            wait_vmcnt_records<(NSTG - 1) * (XTRA == 0 ? LPT : LPT - 1)>(slot);
#pragma unroll
            for (int n = 0; n < NSL; ++n) {
                const uint32_t vi = slot[n] >> 13;                                         // (an empty slot's is past every KV)
                const bool mine = (NG * PACK12_SLOTS >= 64 || (lane >> 3) < NG) && vi < (uint32_t)KV && ((vi >> 3) & 3u) == (uint32_t)wave;
                key[n] = mine ? vi >> 5 : PACK12_EMPTY;
                unsigned long long hit = __builtin_amdgcn_ballot_w64(mine);
#pragma nounroll
                while (hit) {
                    const uint32_t st = __builtin_amdgcn_readlane(key[n], __builtin_ctzll(hit));
                    hit &= hit - 1;
                    if (st & 64u) bm1 |= 1ull << (st & 63u); else bm0 |= 1ull << (st & 63u);
                }
            }
        }
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
                    if constexpr (BITS == 12)
                        asm volatile("ds_read_b64 %0, %2\n\tds_read_b32 %1, %3"
                                     : "=&v"(L[s][rg]), "=&v"(nb[s][rg])
                                     : "v"(sbo + olo[s][rg]), "v"(sbo + onib[s][rg]) : "memory");
                    else if constexpr (R == 4)
                        asm volatile("ds_read_b64 %0, %3\n\tds_read_b32 %1, %4\n\tds_read_b32 %2, %5"
                                     : "=&v"(L[s][rg]), "=&v"(nb[s][rg]), "=&v"(S[s][rg])
                                     : "v"(sbo + olo[s][rg]), "v"(sbo + onib[s][rg]), "v"(sbo + osg[s][rg]) : "memory");
                    else
                        asm volatile("ds_read_b64 %0, %3\n\tds_read_b32 %1, %4\n\tds_read_u16 %2, %5"
                                     : "=&v"(L[s][rg]), "=&v"(nb[s][rg]), "=&v"(S[s][rg])
                                     : "v"(sbo + olo[s][rg]), "v"(sbo + onib[s][rg]), "v"(sbo + osg[s][rg]) : "memory");
                }
            }
            if constexpr (BITS == 12) {
                uint32_t w[KSW][RG][4];
                // one wait for all of them, tied to EVERY value it guards: a piece left out is one the compiler may use ahead of the wait
                // (it did: the shift of the second block's nibbles, which then raced the LDS return)
                static_assert(KSW == 2, "the wait below names the pieces of two sub-steps");
                if constexpr (RG == 1)
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(L[0][0]), "+v"(nb[0][0]), "+v"(L[1][0]), "+v"(nb[1][0]) :: "memory");
                else
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(L[0][0]), "+v"(nb[0][0]), "+v"(L[0][RG - 1]), "+v"(nb[0][RG - 1]), "+v"(L[1][0]), "+v"(nb[1][0]),
                                 "+v"(L[1][RG - 1]), "+v"(nb[1][RG - 1]) :: "memory");
#pragma unroll
                for (int s = 0; s < KSW; ++s)
#pragma unroll
                    for (int rg = 0; rg < RG; ++rg) pack12_decode_row((uint32_t)L[s][rg], (uint32_t)(L[s][rg] >> 32), nb[s][rg], hb4, w[s][rg]);
                // the stage's patches, the whole wave in step (the ballot sees active lanes only; nothing here is per-lane control flow):
                // slot by slot the owning lane replaces the high byte of half j & 1 of dword j >> 1 of its fragment, found by a uniform
                // switch over the wave's KSW * RG * 4 dwords (no indexed registers)
                if (((kt & 64 ? bm1 : bm0) >> (kt & 63)) & 1ull) {
#pragma unroll
                    for (int n = 0; n < NSL; ++n) {
                        unsigned long long hit = __builtin_amdgcn_ballot_w64(key[n] == (uint32_t)kt);
#pragma nounroll
                        while (hit) {
                            const int src_lane = __builtin_ctzll(hit);
                            hit &= hit - 1;
                            const uint32_t pt = __builtin_amdgcn_readlane(slot[n], src_lane);
                            const uint32_t vi = pt >> 13, nl = (uint32_t)((src_lane >> 3) + 8 * n) * R + ((pt >> 11) & (uint32_t)(R - 1));
                            const uint32_t sh = (pt & 0x100u) ? 24u : 8u;
                            const uint32_t m = (uint32_t)lane == ((vi & 3u) << 4 | (nl & 15u)) ? 0xffu << sh : 0u, high = (pt & 0xffu) << sh;
                            const uint32_t at = (((vi >> 2) & 1u) * RG + (nl >> 4)) * 4 + ((pt >> 9) & 3u);
#pragma unroll
                            for (int s = 0; s < KSW; ++s)
#pragma unroll
                                for (int rg = 0; rg < RG; ++rg)
#pragma unroll
                                    for (int d = 0; d < 4; ++d)
                                        if (at == (uint32_t)((s * RG + rg) * 4 + d)) w[s][rg][d] = (w[s][rg][d] & ~m) | (high & m);
                        }
                    }
                }
#pragma unroll
                for (int s = 0; s < KSW; ++s)
#pragma unroll
                    for (int rg = 0; rg < RG; ++rg) af[s][rg] = __builtin_bit_cast(bf16x8_t, u32x4{w[s][rg][0], w[s][rg][1], w[s][rg][2], w[s][rg][3]});
            } else {
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
#define EMU_PT_CASE(E) case E:                                                                                                          \
        if (p.patch) hipLaunchKernelGGL((pack_thin_kernel<E, R, RN, MR, NSTG, 12>), dim3(pl.grid), dim3(pl.block), 0, s, a, p, groups); \
        else hipLaunchKernelGGL((pack_thin_kernel<E, R, RN, MR, NSTG>), dim3(pl.grid), dim3(pl.block), 0, s, a, p, groups);             \
        break;
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
// only pointers can answer is checked here: the set's four pointers, 16-byte aligned planes (the DMA's unit), x, W, out, res.  The
// set's format picks the twin: p.patch set = the 12-bit one (no sign plane, 16-byte aligned records, hb 0..120, vi clear of the empty
// slot's), else the 13-bit one.
int launch_gemv_pack_thin(const GemvArgs& a, const PackSet& p, const GemvPlan& pl, hipStream_t s) {
    const bool b12 = p.patch != nullptr;
    if (pl.status || pl.family != GEMV_FAM_PACK_THIN || pl.kch != 32 || pl.block != 256) return -22;
    if (!a.x || !a.W || !a.out || !p.lo || !p.nib || (b12 ? p.sign != nullptr : !p.sign) || !p.flags || (a.epi == EPI_RESID && !a.res)) return -22;
    if ((reinterpret_cast<size_t>(p.lo) | reinterpret_cast<size_t>(p.nib) | reinterpret_cast<size_t>(p.sign) | reinterpret_cast<size_t>(p.patch) |
         reinterpret_cast<size_t>(a.x) | reinterpret_cast<size_t>(a.W)) & 15) return -22;
    if (a.M < 4 || a.M > pl.mb || a.K < 256 || (a.K & 255) || a.ldw < a.K || (a.ldw & 7) || (a.ldx & 7) || p.hb < 0 || p.hb > (b12 ? 120 : 112)) return -22;
    if (b12 && (a.K >> 3) >= PACK12_MAX_KV) return -22;
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
