// The packer of the 13-bit lossless bf16 weight format (bf16_pack.h): a max-exponent reduction over the matrix, then one pass that
// writes the three planes and the flag bitmap.  Runs once per matrix at load; byte for byte what emu_amd/bf16pack.py::pack writes.
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

}  // namespace

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
