// The packers of the 13-bit and 12-bit lossless bf16 weight formats (bf16_pack.h).  13 bits: a max-exponent reduction over the matrix, then one pass that
// writes the three planes and the flag bitmap.  Runs once per matrix at load; byte for byte what emu_amd/bf16pack.py::pack writes.
// 12 bits: a histogram pass, the window rule on the host, one pass for the planes and the misses, one that sorts or flags each record;
// byte for byte what bf16pack.py::pack12 writes.
#include "common.h"
#include "kernels.h"
#include "bf16_pack.h"

namespace {

// largest exponent field of the finite weights of W [N, K] (row stride ldw elements) -> *emax (zero at launch)
__global__ __launch_bounds__(256) void pack_emax_kernel(const bf16_t* W, int N, int KV, int ldw, unsigned* emax) {
    __shared__ unsigned smax;
    if (threadIdx.x == 0) smax = 0;
    __syncthreads();
    unsigned mx = 0;
    const size_t total = (size_t)N * KV;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t n = i / KV, vi = i - n * KV;
        const u32x4 v = ld16(W + n * ldw + vi * 8);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const unsigned lo = (v[d] >> 7) & 0xff, hi = (v[d] >> 23) & 0xff;
            if (lo != 0xff && lo > mx) mx = lo;
            if (hi != 0xff && hi > mx) mx = hi;
        }
    }
    atomicMax(&smax, mx);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(emax, smax);
}

// one thread per cell (row group g, vector vi): the R rows' 8 weights each -> low units, nibble dwords, sign bytes; flags (zero at launch)
template <int R>
__global__ __launch_bounds__(256) void pack_planes_kernel(const bf16_t* W, int N, int KV, int ldw, const unsigned* emax, uint32_t* lo,
                                                          uint32_t* nib, uint8_t* sign, uint32_t* flags) {
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t G = pack_groups(N, R);
    if (cell >= G * KV) return;
    const size_t g = cell / KV, vi = cell - g * KV;
    const int hb = pack_hb((int)*emax);
    bool flagged = false;
    uint32_t signs = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t n = g * R + r;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        bool bad = false;
        if (n < (size_t)N) {
            const u32x4 v = ld16(W + n * ldw + vi * 8);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        }
        uint32_t L0, L1, nb, sg;
        pack_encode_row<R>(w, r, hb, L0, L1, nb, sg, bad);
        signs |= sg;
        flagged = flagged || (bad && n < (size_t)N);
        uint32_t* unit = lo + (((g * (R / 2) + (r >> 1)) * KV + vi) * 4) + 2 * (r & 1);
        unit[0] = L0; unit[1] = L1;
        nib[cell * R + r] = nb;
    }
    if constexpr (R == 4) reinterpret_cast<uint32_t*>(sign)[cell] = signs;
    else reinterpret_cast<uint16_t*>(sign)[cell] = (uint16_t)signs;
    if (flagged) atomicOr(&flags[g >> 5], 1u << (g & 31));
}

// ---- the 12-bit format.  128-bin histogram of (w >> 8) & 0x7f over W -> hist (zero at launch): runs of equal bins within a thread's
// vector are merged before they go to the workgroup's LDS bins, the workgroup's bins then to the matrix's.  Only counts are added.
__global__ __launch_bounds__(256) void pack12_hist_kernel(const bf16_t* W, int N, int KV, int ldw, unsigned long long* hist) {
    __shared__ unsigned bins[128];
    if (threadIdx.x < 128) bins[threadIdx.x] = 0;
    __syncthreads();
    const size_t total = (size_t)N * KV;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {      // (< 2^32 / 8 vectors per thread)
        const size_t n = i / KV, vi = i - n * KV;
        const u32x4 v = ld16(W + n * ldw + vi * 8);
        unsigned cur = (v[0] >> 8) & 0x7f, run = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned b = (v[j >> 1] >> (8 + 16 * (j & 1))) & 0x7f;
            if (b != cur) { atomicAdd(&bins[cur], run); cur = b; run = 0; }
            ++run;
        }
        atomicAdd(&bins[cur], run);
    }
    __syncthreads();
    if (threadIdx.x < 128 && bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)bins[threadIdx.x]);
}

// one thread per cell (row group g, vector vi): the R rows' 8 weights each -> low units and nibble dwords; every miss takes the next
// free slot of the group's record (patch: 0xff bytes at launch; count: zero at launch, it goes on counting past the 8 slots)
template <int R>
__global__ __launch_bounds__(256) void pack12_planes_kernel(const bf16_t* W, int N, int KV, int ldw, int hb, uint32_t* lo, uint32_t* nib,
                                                            uint32_t* patch, unsigned* count) {
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t G = pack_groups(N, R);
    if (cell >= G * KV) return;
    const size_t g = cell / KV, vi = cell - g * KV;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t n = g * R + r;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        const bool real = n < (size_t)N;
        if (real) {
            const u32x4 v = ld16(W + n * ldw + vi * 8);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        }
        uint32_t L0, L1, nb, miss;
        pack12_encode_row(w, hb, L0, L1, nb, miss);
        if (!real) nb = miss = 0;                                     // a padding row: nibble 0, no miss
        uint32_t* unit = lo + (((g * (R / 2) + (r >> 1)) * KV + vi) * 4) + 2 * (r & 1);
        unit[0] = L0; unit[1] = L1;
        nib[cell * R + r] = nb;
        while (miss) {
            const int j = __builtin_ctz(miss);
            miss &= miss - 1;
            const unsigned k = atomicAdd(&count[g], 1u);
            if (k < (unsigned)PACK12_SLOTS)
                patch[g * PACK12_SLOTS + k] = pack12_slot((uint32_t)vi, r, j, (w[j >> 1] >> (8 + 16 * (j & 1))) & 0xffu);
        }
    }
}

// one thread per row group: more than 8 misses -> flagged, its record empty; else its slots sorted ascending (the empty ones last)
__global__ __launch_bounds__(256) void pack12_finish_kernel(size_t G, const unsigned* count, uint32_t* patch, uint32_t* flags, unsigned* nflagged) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    uint32_t* rec = patch + g * PACK12_SLOTS;
    if (count[g] > (unsigned)PACK12_SLOTS) {
        for (int s = 0; s < PACK12_SLOTS; ++s) rec[s] = PACK12_EMPTY;
        atomicOr(&flags[g >> 5], 1u << (g & 31));
        atomicAdd(nflagged, 1u);
        return;
    }
    for (int a = 1; a < PACK12_SLOTS; ++a)                           // insertion sort in memory: 8 words, once per matrix
        for (int b = a; b > 0 && rec[b - 1] > rec[b]; --b) { const uint32_t t = rec[b]; rec[b] = rec[b - 1]; rec[b - 1] = t; }
}

}  // namespace

int launch_bf16_pack12(const bf16_t* W, int ldw, int N, int K, int rows, void* lo, void* nib, void* patch, uint32_t* flags, int* hb_out,
                       int* flagged_out, hipStream_t s) {
    if (!W || !lo || !nib || !patch || !flags || !hb_out || !flagged_out || N < 1 || K < 32 || (K & 31) || (rows != 2 && rows != 4) || ldw < K || (ldw & 7))
        return -22;
    const int KV = K >> 3;
    const size_t G = pack_groups(N, rows), cells = G * KV;
    if ((cells + 255) / 256 > 0x7fffffffull || KV >= PACK12_MAX_KV) return -22;
    // scratch: the histogram, the flagged-group counter, then one miss counter per row group
    unsigned long long* scratch = nullptr;
    const size_t scratch_bytes = 129 * sizeof(unsigned long long) + G * sizeof(unsigned);
    if (hipMalloc(&scratch, scratch_bytes) != hipSuccess) return -12;
    unsigned* nflagged = reinterpret_cast<unsigned*>(scratch + 128);
    unsigned* count = reinterpret_cast<unsigned*>(scratch + 129);
    unsigned long long hist[128];
    unsigned host_flagged = 0;
    int st = 0, hb = 0;
    auto ok = [&](hipError_t e) { if (e != hipSuccess && !st) st = (int)e; return e == hipSuccess; };
    if (ok(hipMemsetAsync(scratch, 0, scratch_bytes, s)) && ok(hipMemsetAsync(flags, 0, pack_flag_words(N, rows) * 4, s)) &&
        ok(hipMemsetAsync(patch, 0xff, pack12_patch_bytes(N, rows), s))) {
        const size_t vecs = (size_t)N * KV;
        const int g1 = (int)(vecs / 256 / 8 < 1 ? 1 : vecs / 256 / 8 > 4096 ? 4096 : vecs / 256 / 8);
        hipLaunchKernelGGL(pack12_hist_kernel, dim3(g1), dim3(256), 0, s, W, N, KV, ldw, scratch);
        if (ok(hipGetLastError()) && ok(hipMemcpyAsync(hist, scratch, sizeof(hist), hipMemcpyDeviceToHost, s)) && ok(hipStreamSynchronize(s))) {
            hb = pack12_window(hist);                                  // the window rule runs on the host, stated once (bf16_pack.h)
            const dim3 g2((unsigned)((cells + 255) / 256));
            if (rows == 4)
                hipLaunchKernelGGL(pack12_planes_kernel<4>, g2, dim3(256), 0, s, W, N, KV, ldw, hb, (uint32_t*)lo, (uint32_t*)nib, (uint32_t*)patch, count);
            else
                hipLaunchKernelGGL(pack12_planes_kernel<2>, g2, dim3(256), 0, s, W, N, KV, ldw, hb, (uint32_t*)lo, (uint32_t*)nib, (uint32_t*)patch, count);
            ok(hipGetLastError());
            hipLaunchKernelGGL(pack12_finish_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, G, count, (uint32_t*)patch, flags, nflagged);
            ok(hipGetLastError());
            ok(hipMemcpyAsync(&host_flagged, nflagged, sizeof(unsigned), hipMemcpyDeviceToHost, s));
            ok(hipStreamSynchronize(s));                               // the call waits for its own results (hb and the count go to the host)
        }
    }
    (void)hipFree(scratch);
    if (st) return st;
    *hb_out = hb;
    *flagged_out = (int)host_flagged;
    return 0;
}

int launch_bf16_pack(const bf16_t* W, int ldw, int N, int K, int rows, void* lo, void* nib, void* sign, uint32_t* flags, int* hb_out,
                     hipStream_t s) {
    if (!W || !lo || !nib || !sign || !flags || !hb_out || N < 1 || K < 32 || (K & 31) || (rows != 2 && rows != 4) || ldw < K || (ldw & 7))
        return -22;
    const int KV = K >> 3;
    const size_t cells = pack_groups(N, rows) * KV;
    if ((cells + 255) / 256 > 0x7fffffffull) return -22;
    unsigned* emax = nullptr;
    if (hipMalloc(&emax, sizeof(unsigned)) != hipSuccess) return -12;
    unsigned host_emax = 0;
    int st = 0;
    auto ok = [&](hipError_t e) { if (e != hipSuccess && !st) st = (int)e; return e == hipSuccess; };
    if (ok(hipMemsetAsync(emax, 0, sizeof(unsigned), s)) && ok(hipMemsetAsync(flags, 0, pack_flag_words(N, rows) * 4, s))) {
        const size_t vecs = (size_t)N * KV;
        const int g1 = (int)(vecs / 256 / 8 < 1 ? 1 : vecs / 256 / 8 > 4096 ? 4096 : vecs / 256 / 8);
        hipLaunchKernelGGL(pack_emax_kernel, dim3(g1), dim3(256), 0, s, W, N, KV, ldw, emax);
        const dim3 g2((unsigned)((cells + 255) / 256));
        if (rows == 4)
            hipLaunchKernelGGL(pack_planes_kernel<4>, g2, dim3(256), 0, s, W, N, KV, ldw, emax, (uint32_t*)lo, (uint32_t*)nib, (uint8_t*)sign, flags);
        else
            hipLaunchKernelGGL(pack_planes_kernel<2>, g2, dim3(256), 0, s, W, N, KV, ldw, emax, (uint32_t*)lo, (uint32_t*)nib, (uint8_t*)sign, flags);
        ok(hipGetLastError());
        ok(hipMemcpyAsync(&host_emax, emax, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        ok(hipStreamSynchronize(s));                                   // the call waits for its own result (hb goes to the host)
    }
    (void)hipFree(emax);
    if (st) return st;
    *hb_out = pack_hb((int)host_emax);
    return 0;
}
