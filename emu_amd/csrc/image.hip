// Image front end and back end on the device.
//
// In:  torchvision Resize((S, S), BICUBIC) -> ToTensor -> Normalize on a uint8 RGB image (Emu2/emu/chat.py:35-39,
//      Emu2/emu/diffusion.py:58-63), bit-exact with Pillow's 8-bit ImagingResample: a horizontal pass into a uint8 intermediate over
//      the source rows the vertical pass reads, then a vertical pass; every tap sum is an int32 that starts at 1 << 21, is shifted
//      right by 22 and clipped to 0..255.  The coefficient and bounds tables come from the host (emu_amd/preprocess.py restates
//      Pillow's precompute_coeffs + normalize_coeffs_8bpc), ToTensor + Normalize is a [3, 256] table lookup.
// Out: numpy_to_pil's (x * 255).round().astype(uint8) on the decoded bf16 NCHW image (diffusion.py:214-234), written NHWC.
//
// Shape of the two resample kernels (two launches; a single launch would either recompute the horizontal rows once per vertical
// strip -- vertical windows of neighbouring strips overlap by most of their taps -- or need a grid-wide barrier between the passes):
//   horizontal: one workgroup = a strip of TX outputs x 3 channels over RH source rows.  The strip's coefficients are staged once in
//               LDS (odd row stride: conflict-free), every source row's span is fetched with coalesced dword loads into LDS and read
//               from there by all taps of all outputs of the strip; the three channel lanes of an output share every coefficient read.
//   vertical:   one thread = 4 adjacent bytes of a row (one dword load per source row) x RV adjacent output rows: the union of the
//               RV windows is walked once and every loaded dword feeds the accumulators of all rows whose window holds it (registers,
//               static indices); coefficients are wave-uniform loads.  The bytes are transposed through LDS so that the table lookup
//               writes each colour plane of the NCHW output with coalesced stores.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int IMG_RH = 8;          // source rows per horizontal workgroup
constexpr int IMG_RV = 4;          // output rows per vertical thread
constexpr int IMG_VT = 192;        // vertical workgroup: 192 threads x 4 bytes = 256 pixels x 3 channels
constexpr int IMG_LDS_MAX = 60 * 1024;

__device__ __forceinline__ uint32_t clip8(int acc) {
    const int v = acc >> 22;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// 4 bytes at p (any alignment); only the first nvalid are read
__device__ __forceinline__ uint32_t ld_bytes4(const uint8_t* p, int nvalid) {
    uint32_t v = 0;
    if (nvalid >= 4) {
        __builtin_memcpy(&v, p, 4);
    } else {
        for (int b = 0; b < nvalid; ++b) v |= (uint32_t)p[b] << (8 * b);
    }
    return v;
}

__global__ __launch_bounds__(192) void image_resample_h_kernel(
        const uint8_t* __restrict__ src, long pitch, int H, int W, const int32_t* __restrict__ coef,
        const int32_t* __restrict__ bounds, int hk, int S, int row0, int nrows, uint8_t* __restrict__ tmp, int tpitch,
        int TX, int kstride, int span_cap) {
    extern __shared__ uint32_t img_smem[];
    int32_t* cs = reinterpret_cast<int32_t*>(img_smem);                       // [TX][kstride]
    uint32_t* spw = img_smem + TX * kstride;                                  // span_cap bytes of one source row
    const uint8_t* sp = reinterpret_cast<const uint8_t*>(spw);
    const int nt = blockDim.x, t = threadIdx.x;
    const int x0 = blockIdx.x * TX;
    const int nx = min(TX, S - x0);
    for (int i = t; i < nx * hk; i += nt) {
        const int xl = i / hk, k = i - xl * hk;
        cs[xl * kstride + k] = coef[(size_t)x0 * hk + i];
    }
    // the strip's source span [s0, s1): bounds are monotonic in x; everything read from the tables is clamped into the image
    const int last = x0 + nx - 1;
    const int s0 = min(max(bounds[2 * x0], 0), W);
    int s1 = min(max(bounds[2 * last] + bounds[2 * last + 1], s0), W);
    s1 = min(s1, s0 + (span_cap - 8) / 3);
    const int nb = (s1 - s0) * 3;
    const int xl = t / 3, c = t - 3 * xl;
    const bool active = xl < nx;
    int xmin = 0, n = 0;
    if (active) {
        xmin = min(max(bounds[2 * (x0 + xl)], s0), s1);
        n = min(max(bounds[2 * (x0 + xl) + 1], 0), min(hk, s1 - xmin));
    }
    const uint8_t* img_end = src + (size_t)(H - 1) * pitch + (size_t)W * 3;
    const int yend = row0 + nrows;
    for (int ry = 0; ry < IMG_RH; ++ry) {
        const int y = row0 + blockIdx.y * IMG_RH + ry;
        if (y >= yend) break;                                                  // uniform
        const uint8_t* g0 = src + (size_t)y * pitch + (size_t)s0 * 3;
        const int shift = (int)(reinterpret_cast<uintptr_t>(g0) & 3);
        const uint8_t* a = g0 - shift;
        const int ndw = (shift + nb + 3) >> 2;
        __syncthreads();                                                       // the previous row's taps are done (first row: cs is staged)
        for (int i = t; i < ndw; i += nt) {
            const uint8_t* p = a + 4 * (size_t)i;
            uint32_t v = 0;
            if (p >= src && p + 4 <= img_end) {
                v = *reinterpret_cast<const uint32_t*>(p);
            } else {
                for (int b = 0; b < 4; ++b)
                    if (p + b >= src && p + b < img_end) v |= (uint32_t)p[b] << (8 * b);
            }
            spw[i] = v;
        }
        __syncthreads();
        if (active) {
            int acc = 1 << 21;
            const uint8_t* pp = sp + shift + (xmin - s0) * 3 + c;
            const int32_t* cc = cs + xl * kstride;
            for (int k = 0; k < n; ++k) acc += (int)pp[3 * k] * cc[k];
            tmp[(size_t)(y - row0) * tpitch + (x0 + xl) * 3 + c] = (uint8_t)clip8(acc);
        }
    }
}

// in: rows of S * 3 bytes; row r of the image is at in + (r - rbase) * pitch.  SKIP: the vertical pass is the identity (H == S).
template <bool SKIP, bool F32>
__global__ __launch_bounds__(IMG_VT) void image_resample_v_kernel(
        const uint8_t* __restrict__ in, long pitch, int rbase, int rlo, int rhi, const int32_t* __restrict__ coef,
        const int32_t* __restrict__ bounds, int vk, int S, const float* __restrict__ lut, void* __restrict__ out) {
    __shared__ uint32_t tile[IMG_RV][IMG_VT];
    __shared__ float slut[3 * 256];
    const int t = threadIdx.x;
    for (int i = t; i < 3 * 256; i += IMG_VT) slut[i] = lut[i];
    const int rowbytes = S * 3;
    const int col = blockIdx.x * (IMG_VT * 4) + t * 4;
    const int nvalid = min(max(rowbytes - col, 0), 4);
    const int y0 = blockIdx.y * IMG_RV;
    if (SKIP) {
#pragma unroll
        for (int j = 0; j < IMG_RV; ++j) {
            const int y = y0 + j;
            tile[j][t] = (y < S && nvalid > 0) ? ld_bytes4(in + (size_t)(y - rbase) * pitch + col, nvalid) : 0u;
        }
    } else {
        int ymin[IMG_RV], n[IMG_RV], acc[IMG_RV][4];
        int rb = rhi, re = rlo;
#pragma unroll
        for (int j = 0; j < IMG_RV; ++j) {
            const int y = y0 + j;
            ymin[j] = rlo; n[j] = 0;
            if (y < S) {                                                      // uniform; table values clamped into [rlo, rhi)
                ymin[j] = min(max(bounds[2 * y], rlo), rhi);
                n[j] = min(max(bounds[2 * y + 1], 0), min(vk, rhi - ymin[j]));
                if (n[j] > 0) { rb = min(rb, ymin[j]); re = max(re, ymin[j] + n[j]); }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[j][b] = 1 << 21;
        }
        if (nvalid > 0) {
            for (int r = rb; r < re; ++r) {
                const uint32_t v = ld_bytes4(in + (size_t)(r - rbase) * pitch + col, nvalid);
                const int b0 = v & 255, b1 = (v >> 8) & 255, b2 = (v >> 16) & 255, b3 = v >> 24;
#pragma unroll
                for (int j = 0; j < IMG_RV; ++j) {
                    const int k = r - ymin[j];
                    if ((unsigned)k < (unsigned)n[j]) {                       // uniform
                        const int w = coef[(size_t)(y0 + j) * vk + k];
                        acc[j][0] += b0 * w; acc[j][1] += b1 * w; acc[j][2] += b2 * w; acc[j][3] += b3 * w;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < IMG_RV; ++j)
            tile[j][t] = clip8(acc[j][0]) | (clip8(acc[j][1]) << 8) | (clip8(acc[j][2]) << 16) | (clip8(acc[j][3]) << 24);
    }
    __syncthreads();
    // tile[j] holds 256 pixels x 3 interleaved bytes; write them plane by plane, x fastest
    const int px0 = blockIdx.x * (IMG_VT * 4 / 3);
    for (int i = t; i < IMG_RV * 3 * 256; i += IMG_VT) {
        const int x = i & 255, c = (i >> 8) % 3, j = i / 768;
        const int px = px0 + x, y = y0 + j;
        if (px < S && y < S) {
            const uint32_t v = reinterpret_cast<const uint8_t*>(tile[j])[x * 3 + c];
            const float f = slut[c * 256 + v];
            const size_t o = ((size_t)c * S + y) * S + px;
            if (F32) reinterpret_cast<float*>(out)[o] = f;
            else reinterpret_cast<bf16_t*>(out)[o] = f2bf(f);
        }
    }
}

__device__ __forceinline__ uint32_t to_u8(bf16_t x) {
    const float v = rintf(bf2f(x) * 255.0f);                                  // round half to even, as numpy's round
    return (uint32_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);                      // NaN -> 0
}

// bf16 [N, C, HW] -> uint8 [N, HW, C], C <= 4.  VEC: C == 3 and HW % 4 == 0, one thread = 4 pixels (3 x 8-byte loads, 3 dword stores)
template <bool VEC>
__global__ __launch_bounds__(256) void image_to_u8_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ out, int C, long HW,
                                                          long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        if (i >= total) return;                                               // total = N * HW / 4
        const long n = i / (HW >> 2), p = (i - n * (HW >> 2)) << 2;
        const bf16_t* base = x + n * 3 * HW + p;
        uint32_t b[12];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const u32x2 w = *reinterpret_cast<const u32x2*>(base + c * HW);
            b[c] = to_u8((bf16_t)(w.x & 0xffff)); b[3 + c] = to_u8((bf16_t)(w.x >> 16));
            b[6 + c] = to_u8((bf16_t)(w.y & 0xffff)); b[9 + c] = to_u8((bf16_t)(w.y >> 16));
        }
        uint32_t* o = reinterpret_cast<uint32_t*>(out + (n * HW + p) * 3);
#pragma unroll
        for (int d = 0; d < 3; ++d) o[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
    } else {
        if (i >= total) return;                                               // total = N * HW
        const long n = i / HW, p = i - n * HW;
        for (int c = 0; c < C; ++c) out[i * C + c] = (uint8_t)to_u8(x[(n * C + c) * HW + p]);
    }
}

int align_up_i(int v, int a) { return (v + a - 1) / a * a; }

// strip width of the horizontal pass: the widest whose coefficients and source span fit in LDS; 0 = none does
int pick_tx(int W, int S, int hk, int* kstride, int* span_cap) {
    *kstride = hk | 1;
    for (int tx = 64; tx >= 8; tx >>= 1) {
        long span = ((long)(tx - 1) * W + S - 1) / S + hk + 2;
        if (span > W) span = W;
        const long cap = (span * 3 + 8 + 3) / 4 * 4;
        if ((long)tx * *kstride * 4 + cap <= IMG_LDS_MAX) { *span_cap = (int)cap; return tx; }
    }
    return 0;
}

bool resample_shape_ok(int H, int W, int S, int hk, int vk) {
    if (H < 1 || W < 1 || S < 1 || H > EMU_IMAGE_MAX_SIDE || W > EMU_IMAGE_MAX_SIDE || S > EMU_IMAGE_MAX_OUT) return false;
    if (W != S && (hk < 1 || hk > EMU_IMAGE_MAX_TAPS)) return false;
    if (H != S && (vk < 1 || vk > EMU_IMAGE_MAX_TAPS)) return false;
    int ks, cap;
    return W == S || pick_tx(W, S, hk, &ks, &cap) != 0;
}

}  // namespace

size_t image_resample_ws_bytes(int H, int W, int S) {
    if (H < 1 || W < 1 || S < 1 || H > EMU_IMAGE_MAX_SIDE || W > EMU_IMAGE_MAX_SIDE || S > EMU_IMAGE_MAX_OUT) return 0;
    return W == S ? 0 : (size_t)H * align_up_i(S * 3, 16);
}

int launch_image_resample_norm(const ImageResampleArgs& a, hipStream_t s) {
    const int H = a.H, W = a.W, S = a.S;
    if (!resample_shape_ok(H, W, S, a.hk, a.vk) || a.pitch < (long)W * 3 || !a.src || !a.out || !a.lut) return -22;
    const bool horiz = W != S, vert = H != S;
    int row0 = 0, nrows = H;                                                  // rows the horizontal pass makes = rows the vertical pass reads
    if (vert) {
        row0 = a.row0; nrows = a.nrows;
        if (row0 < 0 || nrows < 1 || row0 + nrows > H || !a.vcoef || !a.vbounds) return -22;
    }
    const uint8_t* vin = a.src;
    long vpitch = a.pitch;
    int rbase = 0;
    if (horiz) {
        const int tpitch = align_up_i(S * 3, 16);
        if (!a.hcoef || !a.hbounds || !a.ws || a.ws_bytes < (size_t)nrows * tpitch) return -22;
        int kstride, span_cap;
        const int tx = pick_tx(W, S, a.hk, &kstride, &span_cap);
        const size_t lds = (size_t)tx * kstride * 4 + span_cap;
        hipLaunchKernelGGL(image_resample_h_kernel, dim3((S + tx - 1) / tx, (nrows + IMG_RH - 1) / IMG_RH), dim3(tx * 3), lds, s,
                           a.src, a.pitch, H, W, a.hcoef, a.hbounds, a.hk, S, row0, nrows, static_cast<uint8_t*>(a.ws), tpitch,
                           tx, kstride, span_cap);
        EMU_CHECK_LAUNCH();
        vin = static_cast<const uint8_t*>(a.ws); vpitch = tpitch; rbase = row0;
    }
    const dim3 grid((S * 3 + IMG_VT * 4 - 1) / (IMG_VT * 4), (S + IMG_RV - 1) / IMG_RV);
#define IMG_V(SKIP, F32) hipLaunchKernelGGL((image_resample_v_kernel<SKIP, F32>), grid, dim3(IMG_VT), 0, s, vin, vpitch, rbase, row0, \
                                            row0 + nrows, a.vcoef, a.vbounds, a.vk, S, a.lut, a.out)
    if (vert) { if (a.out_is_f32) IMG_V(false, true); else IMG_V(false, false); }
    else { if (a.out_is_f32) IMG_V(true, true); else IMG_V(true, false); }
#undef IMG_V
    EMU_CHECK_LAUNCH();
    return 0;
}

int launch_image_to_u8(const bf16_t* x, uint8_t* out, int N, int C, int H, int W, hipStream_t s) {
    if (N < 1 || C < 1 || C > 4 || H < 1 || W < 1 || H > EMU_IMAGE_MAX_SIDE || W > EMU_IMAGE_MAX_SIDE || !x || !out) return -22;
    const long HW = (long)H * W;
    if (C == 3 && HW % 4 == 0) {
        const long total = (long)N * (HW / 4);
        if ((total + 255) / 256 > 0x7fffffffL) return -22;
        hipLaunchKernelGGL(image_to_u8_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, out, C, HW, total);
    } else {
        const long total = (long)N * HW;
        if ((total + 255) / 256 > 0x7fffffffL) return -22;
        hipLaunchKernelGGL(image_to_u8_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, out, C, HW, total);
    }
    EMU_CHECK_LAUNCH();
    return 0;
}
