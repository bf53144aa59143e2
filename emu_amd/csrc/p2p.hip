// One-shot peer-to-peer all-reduce for the tensor-parallel decoder's small messages (decode: 13 KB per all-reduce, 120 per
// token) over xGMI, instead of 120 latency-bound RCCL collectives per token.
//
// Every rank owns one COMM BLOCK in its own HBM (uncached, exported with hipIpcGetMemHandle and mapped by every peer):
// two data slots of P2P_SLOT_BYTES and 64-bit flags per slot.  A message is cut into 8 KiB pieces, one workgroup and one
// 16-byte vector per lane each (13 KB = 2 workgroups, 256 KiB = 32), and every piece runs the protocol on its own counter,
// flag and slot region.  All-reduce number s of a piece (a device-side counter, so a captured hipGraph replays correctly)
// uses slot s & 1:
//   1. copy my partial vector into MY slot with system-scope (write-through) stores, wait for their acknowledgement, flag[slot] = s;
//   2. for every rank r in rank order (my own included): wait until r's flag[slot] >= s, read r's slot over xGMI with
//      system-scope loads, add in fp32 -- the same order on every rank, so all ranks hold bit-identical sums;
//   3. round to bf16 in place.
// Point-to-point xGMI means every rank reads the other N - 1 vectors directly (N - 1 links busy per rank, one hop, no
// ring): for 13 KB the cost is one flag round trip + one remote read, not 2 (N - 1) ring steps.
// Slot reuse is safe with two slots: a rank rewrites slot s & 1 at all-reduce s + 2, which it reaches only after finishing
// s + 1, which needed every peer's s + 1 vector, which a peer publishes only after its reads of all-reduce s are done.
// Every wait is BOUNDED in wall-clock time (s_memrealtime, 100 MHz): past the limit a give-up counter is raised, the kernel
// proceeds, and every later all-reduce skips its wait, so a dead peer or a platform problem costs one time-out, never a hung
// GPU.  The host reads the counter (emu_tp_p2p_giveups) after the self-test at initialisation -- a failed self-test keeps the
// path on RCCL -- and after every generation, where a non-zero count is an error (the sums are garbage).
// Messages larger than a slot go through it in chunks (tests on one GPU); production sends them to RCCL (engine.hip).
//
// Replaces (with emu_amd/tp.py) the reference's layer-placement "model parallel": Emu2/emu/mixin.py:14-85, chat.py:235-283.
#include <string.h>

#include "common.h"
#include "kernels.h"

namespace {

__device__ unsigned int g_p2p_giveups = 0;

struct P2pPeers {
    char* block[EMU_P2P_MAX_RANKS];                 // every rank's comm block as mapped in THIS process (own block included)
    int n, rank;
    long long limit_ticks;                          // wait bound in s_memrealtime ticks (100 MHz)
    int fenced;                                     // 1: the exchange is bracketed by two system-scope fences (see the kernel)
};

// piece g of a message: elements [g * P2P_PIECE, (g + 1) * P2P_PIECE), one 16-byte vector per lane of workgroup g, which runs
// its own instance of the protocol (own sequence counter, own flag per slot, own 8 KiB of each slot)
constexpr int P2P_PIECE = EMU_P2P_PIECE;
constexpr int P2P_PIECES = EMU_P2P_PIECES;

__device__ __forceinline__ unsigned long long* flag_of(char* block, int slot, int g) {
    return reinterpret_cast<unsigned long long*>(block + 2 * EMU_P2P_SLOT_BYTES) + slot * P2P_PIECES + g;
}

__global__ __launch_bounds__(512) void p2p_allreduce_kernel(P2pPeers p, unsigned long long* seq_counter, bf16_t* x, int n) {
    __shared__ unsigned long long s_sh;
    const int tid = threadIdx.x, g = blockIdx.x;
    const int e0 = g * P2P_PIECE + tid * 8;                                 // my 8 elements
    const bool full = e0 + 8 <= n, part = e0 < n;
    // my share of the partial vector is requested BEFORE the sequence counter makes its round trip through LDS (round 6: the two
    // loads were two dependent trips of a launch that is nothing but dependent trips)
    u32x4 mine = {0u, 0u, 0u, 0u};
    if (full) mine = ld16(x + e0);
    if (tid == 0) { s_sh = seq_counter[g] + 1; seq_counter[g] = s_sh; }   // launches of one stream are ordered: no race
    __syncthreads();
    const unsigned long long s = s_sh;
    const int slot = (int)(s & 1);
    const size_t off = (size_t)slot * EMU_P2P_SLOT_BYTES + (size_t)e0 * 2;
    // Two forms of the exchange, chosen per launch (P2pPeers::fenced):
    //  * fenced (the default of a fresh comm block): the HIP memory model's own release / acquire -- __threadfence_system() between
    //    the payload stores and the flag, and again between the last flag poll and the payload loads.  ~3.5 us each of a 6.8 us launch.
    //  * fence-free (round 5): no cache-wide operation at all.  The slot is written with system-scope (sc0 sc1, write-through) stores
    //    whose acknowledgement the wave waits for before the flag goes out, and read with system-scope loads, which no cache level
    //    serves -- MI355X_MICROARCH.md's "{sc0 sc1 stores and loads both sides}" form.  That rests on gfx950's write-through / ack
    //    behaviour, not on the memory model, and ranks that share one GPU (every run this repository has had) share an L2 and never
    //    exercise xGMI -- so the host switches it on only after a SOAK of this form passed on every rank of the job it is about to
    //    serve (emu_amd/llama.py::_init_p2p: hundreds of back-to-back all-reduces of sequence-dependent data, every word checked).
    // Both forms use the same sc0 sc1 stores and loads, so the fences are purely additional ordering.
    const __amdgpu_buffer_rsrc_t rmine = __builtin_amdgcn_make_buffer_rsrc(p.block[p.rank], 0, (uint32_t)(2 * EMU_P2P_SLOT_BYTES), 0x00020000);
    // ---- 1. publish my piece
    if (part) {
        u32x4 v;
        if (full) v = mine;
        else {
            bf16_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int j = 0; e0 + j < n; ++j) t[j] = x[e0 + j];
            v = *reinterpret_cast<u32x4*>(t);
        }
        __builtin_amdgcn_raw_buffer_store_b128(v, rmine, (uint32_t)off, 0, 17);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                      // this wave's share has reached the system's point of coherence
    if (p.fenced) __threadfence_system();                                  // release
    __syncthreads();
    if (tid == 0) __hip_atomic_store(flag_of(p.block[p.rank], slot, g), s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // ---- 2. wait for every rank's piece of this sequence number
    if (tid < p.n) {
        unsigned long long* f = flag_of(p.block[tid], slot, g);
        const bool dead = __hip_atomic_load(&g_p2p_giveups, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        const long long t0 = wall_clock64();
        while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < s) {
            if (dead || wall_clock64() - t0 > p.limit_ticks) { atomicAdd(&g_p2p_giveups, 1u); break; }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    if (p.fenced) __threadfence_system();                                  // acquire (every wave: the loads below are its own)
    __syncthreads();
    // ---- 3. sum in rank order, fp32
    if (part) {
        u32x4 v[EMU_P2P_MAX_RANKS];
#pragma unroll
        for (int r = 0; r < EMU_P2P_MAX_RANKS; ++r)
            if (r < p.n)
                v[r] = __builtin_amdgcn_raw_buffer_load_b128(
                    __builtin_amdgcn_make_buffer_rsrc(p.block[r], 0, (uint32_t)(2 * EMU_P2P_SLOT_BYTES), 0x00020000), (uint32_t)off, 0, 17);
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < EMU_P2P_MAX_RANKS; ++r)
            if (r < p.n) {
                float f[8];
                unpack8(v[r], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += f[j];
            }
        if (full) st16(x + e0, pack8(acc));
        else for (int j = 0; e0 + j < n; ++j) x[e0 + j] = f2bf(acc[j]);
    }
}

}  // namespace

static size_t emu_p2p_engine_offset() {
    return (2 * EMU_P2P_SLOT_BYTES + 2 * P2P_PIECES * sizeof(unsigned long long) + 255) / 256 * 256;
}
constexpr int EMU_ENG_SEQ_WORDS = 1024;           // per-CU all-reduce counters of the engine (>= CUs of any device)

struct EmuP2p {
    char* mine = nullptr;                           // my comm block (device memory owned by this object)
    char* block[EMU_P2P_MAX_RANKS] = {};
    bool opened[EMU_P2P_MAX_RANKS] = {};
    unsigned long long* seq = nullptr;              // device-side sequence counters, one per piece (plain device memory)
    unsigned int* eng_seq = nullptr;                // decode_engine.hip: all-reduces every CU has been through (plain device memory)
    int n = 0, rank = 0;
    long long limit_ticks = 10LL * 100000000LL;     // 10 s
    int fenced = 1;                                 // emu_p2p_set_fenced: the memory-model form until the host's soak cleared the other
};

EmuP2p* emu_p2p_create(int rank, int n, void* handle64_out) {
    if (n < 1 || n > EMU_P2P_MAX_RANKS || rank < 0 || rank >= n) return nullptr;
    EmuP2p* p = new EmuP2p();
    p->n = n; p->rank = rank;
    const size_t bytes = emu_p2p_engine_offset() + EMU_P2P_ENG_BYTES;      // [slot 0 | slot 1 | flags | engine area (decode_engine.hip)]
    void* ptr = nullptr;
    // uncached (what RCCL uses for its own peer-visible buffers on gfx94x/gfx950), else fine-grained, else plain device memory:
    // the kernel's system-scope release / acquire pairs are sufficient for any of the three.
    if (hipExtMallocWithFlags(&ptr, bytes, hipDeviceMallocUncached) != hipSuccess) {
        (void)hipGetLastError();
        if (hipExtMallocWithFlags(&ptr, bytes, hipDeviceMallocFinegrained) != hipSuccess) {
            (void)hipGetLastError();
            if (hipMalloc(&ptr, bytes) != hipSuccess) { delete p; return nullptr; }
        }
    }
    p->mine = reinterpret_cast<char*>(ptr);
    if (hipMemset(p->mine, 0, bytes) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&p->seq), P2P_PIECES * 8) != hipSuccess ||
        hipMemset(p->seq, 0, P2P_PIECES * 8) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&p->eng_seq), EMU_ENG_SEQ_WORDS * 4) != hipSuccess ||
        hipMemset(p->eng_seq, 0, EMU_ENG_SEQ_WORDS * 4) != hipSuccess) { emu_p2p_destroy(p); return nullptr; }
    (void)hipDeviceSynchronize();
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle is 64 bytes");
    hipIpcMemHandle_t h;
    if (hipIpcGetMemHandle(&h, p->mine) != hipSuccess) { emu_p2p_destroy(p); return nullptr; }
    memcpy(handle64_out, &h, 64);
    p->block[rank] = p->mine;
    return p;
}

int emu_p2p_open(EmuP2p* p, const void* handles) {
    if (!p || !handles) return -22;
    for (int r = 0; r < p->n; ++r) {
        if (r == p->rank) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, reinterpret_cast<const char*>(handles) + 64 * r, 64);
        void* ptr = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) return (int)e;
        p->block[r] = reinterpret_cast<char*>(ptr);
        p->opened[r] = true;
    }
    return 0;
}

void emu_p2p_destroy(EmuP2p* p) {
    if (!p) return;
    for (int r = 0; r < p->n; ++r)
        if (p->opened[r]) (void)hipIpcCloseMemHandle(p->block[r]);
    if (p->mine) (void)hipFree(p->mine);
    if (p->seq) (void)hipFree(p->seq);
    if (p->eng_seq) (void)hipFree(p->eng_seq);
    delete p;
}

int emu_p2p_allreduce(EmuP2p* p, bf16_t* x, size_t n, hipStream_t s) {
    if (!p || !x) return -22;
    for (int r = 0; r < p->n; ++r)
        if (!p->block[r]) return -107;                                     // peers not mapped yet
    P2pPeers peers;
    for (int r = 0; r < EMU_P2P_MAX_RANKS; ++r) peers.block[r] = r < p->n ? p->block[r] : nullptr;
    peers.n = p->n; peers.rank = p->rank; peers.limit_ticks = p->limit_ticks; peers.fenced = p->fenced;
    const size_t chunk = EMU_P2P_SLOT_BYTES / 2;                           // elements per slot
    for (size_t o = 0; o < n; o += chunk) {
        const int m = (int)(n - o < chunk ? n - o : chunk);
        hipLaunchKernelGGL(p2p_allreduce_kernel, dim3((m + P2P_PIECE - 1) / P2P_PIECE), dim3(512), 0, s, peers, p->seq, x + o, m);
    }
    EMU_CHECK_LAUNCH();
    return 0;
}

bool emu_p2p_view(EmuP2p* p, char** block8, unsigned long long** seq, int* n, int* rank, long long* limit_ticks) {
    if (!p) return false;
    for (int r = 0; r < p->n; ++r)
        if (!p->block[r]) return false;
    for (int r = 0; r < EMU_P2P_MAX_RANKS; ++r) block8[r] = r < p->n ? p->block[r] : nullptr;
    *seq = p->seq; *n = p->n; *rank = p->rank; *limit_ticks = p->limit_ticks;
    return true;
}

bool emu_p2p_engine_view(EmuP2p* p, char** area8, unsigned int** seq, int* n, int* rank) {
    if (!p || !p->eng_seq) return false;
    for (int r = 0; r < p->n; ++r)
        if (!p->block[r]) return false;
    for (int r = 0; r < EMU_P2P_MAX_RANKS; ++r) area8[r] = r < p->n ? p->block[r] + emu_p2p_engine_offset() : nullptr;
    *seq = p->eng_seq; *n = p->n; *rank = p->rank;
    return true;
}

void emu_p2p_set_fenced(EmuP2p* p, int fenced) { if (p) p->fenced = fenced != 0; }
int emu_p2p_fenced(const EmuP2p* p) { return p ? p->fenced : -1; }
void emu_p2p_set_timeout_ms(EmuP2p* p, int ms) { if (p && ms > 0) p->limit_ticks = (long long)ms * 100000LL; }

unsigned int emu_p2p_giveups_read() {
    unsigned int v = 0;
    (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_p2p_giveups), sizeof v);
    return v;
}

// =============================================================================================== ViT token-row exchange
// Token-parallel ViT encode of one image (engine.hip: emu_vit_forward_tp): rank r computes token rows [rows[r], rows[r + 1]) of
// every block and needs every rank's K rows and V^T key columns before its attention.  Every rank owns one EXCHANGE REGION in
// its own HBM (allocated, exported and mapped like the comm block above): two sets [A: N x wa | B: wb x ldb] used alternately,
// then 64-bit flags per set and piece.  One launch = one exchange, VITX_PIECES workgroups, each running the protocol of
// p2p_allreduce_kernel on its own piece (device-side sequence counter, flag per set, bounded waits, shared give-up counter,
// fenced or fence-free form):
//   1. publish: copy my rows of A (token-major: K rows, or the final [N, C] tokens) and my 8-key groups of B (token-minor: V^T)
//      that belong to piece g into MY region's set s & 1 with system-scope stores, wait for their acknowledgement, flag = s;
//   2. for every peer: wait until its flag of piece g reaches s, copy its rows of piece g from its region into my local A / B.
// Piece g of rank q is A rows [rows[q] + g * ceil(n_q / P), ...) and B rows [g * ceil(wb / P), ...) at rank q's keys: every rank
// derives every peer's pieces from the common row partition, so a zero-row rank publishes nothing and still flags and pulls.
// Set reuse is safe with two sets for the all-reduce's reason: a rank rewrites set s & 1 at exchange s + 2, which it reaches only
// after exchange s + 1, which needed every peer's flag of s + 1, raised only after that peer's launch of exchange s had finished.
namespace {

struct VitXArgs {
    char* region[EMU_P2P_MAX_RANKS];                // every rank's exchange region as mapped in THIS process
    int rows[EMU_P2P_MAX_RANKS + 1];                // token row partition (emu_amd/tp.py::token_rows)
    int n, rank, fenced;
    long long limit_ticks;
    bf16_t* a; int lda, wa;                         // local token-major matrix: row t at a + t * lda, wa columns (multiple of 8)
    bf16_t* b; int ldb, wb;                         // local token-minor matrix (null: none): row j at b + j * ldb, keys in 8-groups
    uint32_t set_bytes, b_off, flag_off, region_bytes;
};

__device__ __forceinline__ void vitx_rows_of(const VitXArgs& p, int q, int g, int& t0, int& t1, int& k0, int& k1, int& j0, int& j1) {
    const int r0 = p.rows[q], r1 = p.rows[q + 1], nr = r1 - r0;
    const int per = (nr + VITX_PIECES - 1) / VITX_PIECES;
    t0 = min(r0 + g * per, r1); t1 = min(t0 + per, r1);
    k0 = r0 >> 3; k1 = nr > 0 ? (r1 + 7) >> 3 : k0;                       // 8-key groups (the last rank's ragged group included)
    const int perb = (p.wb + VITX_PIECES - 1) / VITX_PIECES;
    j0 = min(g * perb, p.wb); j1 = min(j0 + perb, p.wb);
}

__global__ __launch_bounds__(256) void vit_row_exchange_kernel(VitXArgs p, unsigned long long* seq_counter) {
    __shared__ unsigned long long s_sh;
    const int tid = threadIdx.x, g = blockIdx.x;
    if (tid == 0) { s_sh = seq_counter[g] + 1; seq_counter[g] = s_sh; }   // launches of one stream are ordered: no race
    __syncthreads();
    const unsigned long long s = s_sh;
    const int set = (int)(s & 1);
    const uint32_t abase = (uint32_t)set * p.set_bytes, bbase = abase + p.b_off;
    const int av = p.wa >> 3;                                              // 16-byte vectors per A row
    // ---- 1. publish my piece (the same sc0 sc1 stores in both forms; fenced adds the system-scope release)
    {
        int t0, t1, k0, k1, j0, j1;
        vitx_rows_of(p, p.rank, g, t0, t1, k0, k1, j0, j1);
        const __amdgpu_buffer_rsrc_t rmine = __builtin_amdgcn_make_buffer_rsrc(p.region[p.rank], 0, p.region_bytes, 0x00020000);
        for (int i = tid; i < (t1 - t0) * av; i += 256) {
            const int t = t0 + i / av, c = (i % av) * 8;
            __builtin_amdgcn_raw_buffer_store_b128(ld16(p.a + (size_t)t * p.lda + c), rmine, abase + (uint32_t)(t * p.wa + c) * 2, 0, 17);
        }
        const int kv = k1 - k0;
        if (p.b)
            for (int i = tid; i < (j1 - j0) * kv; i += 256) {
                const int j = j0 + i / kv, k = (k0 + i % kv) * 8;
                __builtin_amdgcn_raw_buffer_store_b128(ld16(p.b + (size_t)j * p.ldb + k), rmine, bbase + (uint32_t)(j * p.ldb + k) * 2, 0, 17);
            }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (p.fenced) __threadfence_system();                                  // release
    __syncthreads();
    unsigned long long* myflag = reinterpret_cast<unsigned long long*>(p.region[p.rank] + p.flag_off) + set * VITX_PIECES + g;
    if (tid == 0) __hip_atomic_store(myflag, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // ---- 2. wait for every peer's piece g of this exchange
    if (tid < p.n && tid != p.rank) {
        unsigned long long* f = reinterpret_cast<unsigned long long*>(p.region[tid] + p.flag_off) + set * VITX_PIECES + g;
        const bool dead = __hip_atomic_load(&g_p2p_giveups, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        const long long t0 = wall_clock64();
        while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < s) {
            if (dead || wall_clock64() - t0 > p.limit_ticks) { atomicAdd(&g_p2p_giveups, 1u); break; }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    if (p.fenced) __threadfence_system();                                  // acquire
    __syncthreads();
    // ---- 3. pull every peer's piece g into my local matrices (system-scope loads: no cache level serves them)
    for (int q = 0; q < p.n; ++q) {
        if (q == p.rank) continue;
        int t0, t1, k0, k1, j0, j1;
        vitx_rows_of(p, q, g, t0, t1, k0, k1, j0, j1);
        const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(p.region[q], 0, p.region_bytes, 0x00020000);
        for (int i = tid; i < (t1 - t0) * av; i += 256) {
            const int t = t0 + i / av, c = (i % av) * 8;
            st16(p.a + (size_t)t * p.lda + c, __builtin_amdgcn_raw_buffer_load_b128(rq, abase + (uint32_t)(t * p.wa + c) * 2, 0, 17));
        }
        const int kv = k1 - k0;
        if (p.b)
            for (int i = tid; i < (j1 - j0) * kv; i += 256) {
                const int j = j0 + i / kv, k = (k0 + i % kv) * 8;
                st16(p.b + (size_t)j * p.ldb + k, __builtin_amdgcn_raw_buffer_load_b128(rq, bbase + (uint32_t)(j * p.ldb + k) * 2, 0, 17));
            }
    }
}

}  // namespace

struct EmuVitX {
    char* mine = nullptr;                           // my exchange region (device memory owned by this object)
    char* region[EMU_P2P_MAX_RANKS] = {};
    bool opened[EMU_P2P_MAX_RANKS] = {};
    unsigned long long* seq = nullptr;              // device-side sequence counters, one per piece
    int n = 0, rank = 0, fenced = 1;
    int a_elems = 0, wb = 0, ldb = 0;               // capacity: A rows x columns (elements), B rows and leading dimension
    uint32_t set_bytes = 0, b_off = 0, flag_off = 0, bytes = 0;
    long long limit_ticks = 10LL * 100000000LL;     // 10 s
};

EmuVitX* emu_vitx_create(int rank, int n, size_t a_elems, int wb, int ldb, void* handle64_out) {
    if (n < 2 || n > EMU_P2P_MAX_RANKS || rank < 0 || rank >= n || wb < 0 || (ldb & 7)) return nullptr;
    const size_t b_off = (a_elems * 2 + 255) / 256 * 256, set = (b_off + (size_t)wb * ldb * 2 + 255) / 256 * 256;
    const size_t bytes = 2 * set + 2 * VITX_PIECES * sizeof(unsigned long long);
    if (bytes >= (1ull << 31)) return nullptr;                            // 32-bit buffer offsets
    EmuVitX* p = new EmuVitX();
    p->n = n; p->rank = rank; p->a_elems = (int)a_elems; p->wb = wb; p->ldb = ldb;
    p->b_off = (uint32_t)b_off; p->set_bytes = (uint32_t)set; p->flag_off = (uint32_t)(2 * set); p->bytes = (uint32_t)bytes;
    void* ptr = nullptr;
    if (hipExtMallocWithFlags(&ptr, bytes, hipDeviceMallocUncached) != hipSuccess) {
        (void)hipGetLastError();
        if (hipExtMallocWithFlags(&ptr, bytes, hipDeviceMallocFinegrained) != hipSuccess) {
            (void)hipGetLastError();
            if (hipMalloc(&ptr, bytes) != hipSuccess) { delete p; return nullptr; }
        }
    }
    p->mine = reinterpret_cast<char*>(ptr);
    if (hipMemset(p->mine, 0, bytes) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&p->seq), VITX_PIECES * 8) != hipSuccess ||
        hipMemset(p->seq, 0, VITX_PIECES * 8) != hipSuccess) { emu_vitx_destroy(p); return nullptr; }
    (void)hipDeviceSynchronize();
    hipIpcMemHandle_t h;
    if (hipIpcGetMemHandle(&h, p->mine) != hipSuccess) { emu_vitx_destroy(p); return nullptr; }
    memcpy(handle64_out, &h, 64);
    p->region[rank] = p->mine;
    return p;
}

int emu_vitx_open(EmuVitX* p, const void* handles, int timeout_ms, int fenced) {
    if (!p || !handles) return -22;
    for (int r = 0; r < p->n; ++r) {
        if (r == p->rank || p->opened[r]) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, reinterpret_cast<const char*>(handles) + 64 * r, 64);
        void* ptr = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) return (int)e;
        p->region[r] = reinterpret_cast<char*>(ptr);
        p->opened[r] = true;
    }
    if (timeout_ms > 0) p->limit_ticks = (long long)timeout_ms * 100000LL;
    p->fenced = fenced != 0;
    return 0;
}

void emu_vitx_destroy(EmuVitX* p) {
    if (!p) return;
    for (int r = 0; r < p->n; ++r)
        if (p->opened[r]) (void)hipIpcCloseMemHandle(p->region[r]);
    if (p->mine) (void)hipFree(p->mine);
    if (p->seq) (void)hipFree(p->seq);
    delete p;
}

int emu_vitx_exchange(EmuVitX* p, const int* rows, bf16_t* a, int lda, int wa, bf16_t* b, int ldb, hipStream_t s) {
    if (!p || !a || (wa & 7) || (lda & 7) || ((uintptr_t)a & 15) || ((uintptr_t)b & 15)) return -22;
    if (rows[0] != 0 || (size_t)rows[p->n] * wa > (size_t)p->a_elems || (b && (ldb != p->ldb || (rows[p->n] + 7) / 8 * 8 > ldb))) return -22;
    for (int r = 0; r < p->n; ++r)
        if (rows[r + 1] < rows[r] || (r > 0 && rows[r] < rows[p->n] && (rows[r] & 7))) return -22;   // ascending, 8-aligned starts
    for (int r = 0; r < p->n; ++r)
        if (!p->region[r]) return -107;                                    // peers not mapped yet
    VitXArgs x;
    for (int r = 0; r < EMU_P2P_MAX_RANKS; ++r) x.region[r] = r < p->n ? p->region[r] : nullptr;
    for (int r = 0; r <= EMU_P2P_MAX_RANKS; ++r) x.rows[r] = rows[r < p->n ? r : p->n];
    x.n = p->n; x.rank = p->rank; x.fenced = p->fenced; x.limit_ticks = p->limit_ticks;
    x.a = a; x.lda = lda; x.wa = wa; x.b = b; x.ldb = p->ldb; x.wb = b ? p->wb : 0;
    x.set_bytes = p->set_bytes; x.b_off = p->b_off; x.flag_off = p->flag_off; x.region_bytes = p->bytes;
    hipLaunchKernelGGL(vit_row_exchange_kernel, dim3(VITX_PIECES), dim3(256), 0, s, x, p->seq);
    EMU_CHECK_LAUNCH();
    return 0;
}
