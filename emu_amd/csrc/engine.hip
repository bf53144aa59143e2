// C ABI of libemu_hip.so (declared in include/emu_hip.h): context + RCCL communicator, primitive operator
// entry points, and the LLaMA / EVA-ViT engines that chain the kernels on one HIP stream without any
// allocation or synchronisation (so whole forwards are hipGraph / stream-capture safe).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/emu_hip.h"
#include "kernels.h"
#include "bf16_pack.h"

struct emu_ctx {
    int device = 0, tp_rank = 0, tp_size = 1;
    int ncu = 0;                                    // compute units of the device (0: the query failed; the persistent engine stays off)
    ncclComm_t comm = nullptr;
    EmuP2p* p2p = nullptr;                          // one-shot all-reduce blocks (p2p.hip); used only once enabled
    bool p2p_on = false;
    // tensor-parallel prefill in two concurrent lanes (emu_llama_set_tp_overlap): the second half of a prompt's rows runs on
    // lane_stream beside the caller's stream; the events chain the two
    hipStream_t lane_stream = nullptr;
    hipEvent_t ar_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    std::string err;
};

namespace {
inline hipStream_t S(emu_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline const bf16_t* B(const void* p) { return reinterpret_cast<const bf16_t*>(p); }
inline bf16_t* B(void* p) { return reinterpret_cast<bf16_t*>(p); }
inline const uint8_t* U8(const void* p) { return reinterpret_cast<const uint8_t*>(p); }
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

int fail(emu_ctx* c, int code, const char* what) {
    if (c) { char buf[256]; snprintf(buf, sizeof buf, "%s (status %d)", what, code); c->err = buf; }
    return code;
}
#define TRY(c, expr) do { int st__ = (expr); if (st__ != 0) return fail((c), st__, #expr); } while (0)

// HIP-event timing of the weight-streaming GEMV launches (bench.py roofline leg; eager mode only)
struct GemvProfiler {
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t used = 0;
    double bytes = 0.0;
} g_prof;

// launch profiler: event pairs + what was launched, aggregated on read
struct LaunchProfiler {
    bool on = false;
    struct Rec { hipEvent_t a, b; const char* klass; int M, N, K, tag; double flops; };
    std::vector<Rec> recs;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    size_t used = 0;
    hipEvent_t cur_a = nullptr, cur_b = nullptr;
} g_lprof;

// a weight-streaming launch between a HIP-event pair of the GEMV profiler when that is on
template <class Launch>
int gemv_profiled(double weight_bytes, hipStream_t s, Launch launch) {
    if (!g_prof.on) return launch();
    if (g_prof.used == g_prof.ev.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -12;
        g_prof.ev.emplace_back(a, b);
    }
    auto& e = g_prof.ev[g_prof.used++];
    g_prof.bytes += weight_bytes;
    (void)hipEventRecord(e.first, s);
    const int st = launch();
    (void)hipEventRecord(e.second, s);
    return st;
}

// ---- The weight sets of one matrix, any of them null: bf16; fp8 (e4m3) bytes + one fp32 scale per output row; MXFP4 element bytes
// [N, K/2] + E8M0 block scales [N, K/32] at a row stride of fp4_scale_stride(K); and the 13-bit lossless packing of the bf16 matrix
// [pkN, pkK] (bf16_pack.h; pk.rows == 0: none), whose flagged row groups read the bf16 rows
struct Weights { const bf16_t* W = nullptr; const uint8_t* W8 = nullptr; const float* s8 = nullptr;
                 const uint8_t* W4 = nullptr; const uint8_t* s4 = nullptr;
                 PackSet pk; int pkN = 0, pkK = 0; };
enum class WeightSet { Bf16, Fp8, Fp4, Pack };
// what a set says of every kernel that reads it: whether the record holds it, K over its weight row stride, and the bytes one pass
// over an [N, K] matrix is priced at under the weight-stream profiler (R: the rows per group of a packed set, priced at what it stores)
bool holds(const Weights& w, WeightSet set) { return set == WeightSet::Bf16 ? w.W != nullptr : set == WeightSet::Fp8 ? w.W8 && w.s8 : set == WeightSet::Fp4 ? w.W4 && w.s4 : w.W && w.pk.rows; }
constexpr int set_kdiv(WeightSet set) { return set == WeightSet::Fp4 ? 2 : 1; }
double set_bytes(WeightSet set, int N, int K, int R = 0, bool twelve = false) {       // twelve: a packed set of the 12-bit format
    if (set == WeightSet::Pack)
        return (double)(pack_lo_bytes(N, K, R) + pack_nib_bytes(N, K, R) + (twelve ? pack12_patch_bytes(N, R) : pack_sign_bytes(N, K, R)) + 4 * pack_flag_words(N, R));
    return set == WeightSet::Fp4 ? (double)N * (double)(K / 2 + K / 32) : (set == WeightSet::Fp8 ? 1.0 : 2.0) * (double)N * (double)K;
}
// The kernels of a LLaMA projection (ABI: the values emu_llama_projection_kernel and its three views return), and what each is, said
// once: the set it reads; the rows it serves; whether it takes the RMSNorm in front; whether a bf16 GEMM runs its calls of 17 rows and
// more -- the one that carries the RoPE epilogue, the K-slice sum + RMSNorm and the two-lane prefill (Fp8Gemm: the W8A8 GEMM beside
// it, on the caller's quantised rows through linear_q8, bf16 in a matrix without an fp8 copy; those fusions are off under it anyway).
enum class WeightKernel { Bf16 = 0, Fp8Rows = 1, Fp8Gemm = 2, Fp4Rows = 3, Fp4Thin = 4, Fp4Gemm = 5, Bf16Pack = 6, Fp8Thin = 7, Bf16PackThin = 8, Fp8Stream = 9, Fp8Tile = 10 };
struct KernelFacts { WeightSet set; int lo, hi; bool norm, bf16_gemm; };
constexpr int ANY_ROWS = 1 << 30;
constexpr KernelFacts KERNEL_FACTS[] = {
    {WeightSet::Bf16, 1, ANY_ROWS, true, true},      // Bf16          gemv.hip up to 8 / 16 rows, the GEMMs above (linear)
    {WeightSet::Fp8, 1, 2, true, false},             // Fp8Rows       gemv.hip
    {WeightSet::Fp8, 17, ANY_ROWS, false, true},     // Fp8Gemm       block-scaled MFMA, twice the bf16 rate (BASELINE configs[4]); whole 128-element k tiles
    {WeightSet::Fp4, 1, 2, true, false},             // Fp4Rows       gemv_fp4.hip; K % 32 == 0
    {WeightSet::Fp4, 1, 16, false, false},           // Fp4Thin       gemv_fp4_thin.hip, matrix cores; K >= 256, K % 32 == 0
    {WeightSet::Fp4, 17, ANY_ROWS, false, false},    // Fp4Gemm       gemm_fp4.hip; the same
    {WeightSet::Pack, 1, 1, true, false},            // Bf16Pack      gemv_pack.hip: the bf16 stream's bits at 13/16 of its bytes
    {WeightSet::Fp8, 1, 16, false, false},           // Fp8Thin       gemv_fp8_thin.hip, matrix cores; whole 256-element k stages
    {WeightSet::Pack, 4, 16, false, false},          // Bf16PackThin  gemv_pack_thin.hip: the packed twin of the bf16 few-row stream
    {WeightSet::Fp8, 17, 64, false, false},          // Fp8Stream     gemm_fp8.hip, W8A16; the same whole stages
    {WeightSet::Fp8, 65, ANY_ROWS, false, false},    // Fp8Tile       gemm_fp8.hip, its 64 x 128 form under the fp8_all switch; the same
};
constexpr const KernelFacts& facts(WeightKernel k) { return KERNEL_FACTS[(int)k]; }
constexpr bool serves(WeightKernel k, int rows) { return rows >= facts(k).lo && rows <= facts(k).hi; }
constexpr bool needs_fp8(WeightKernel k) { return facts(k).set == WeightSet::Fp8 && !facts(k).bf16_gemm; }   // no bf16 to fall back to
constexpr bool norm_rides(WeightKernel k) { return facts(k).norm && facts(k).set != WeightSet::Bf16 && facts(k).set != WeightSet::Pack; }   // in every call
int linear(const bf16_t* A, const bf16_t* W, const bf16_t* bias, const bf16_t* res, const bf16_t* norm_w,
           bf16_t* C, int M, int N, int K, int lda, int ldw, int ldres, int ldc, float eps, int epi, hipStream_t s,
           const float* wscale = nullptr, float* splitk = nullptr, size_t splitk_floats = 0, const WarmPlan* warm = nullptr) {
    if (wscale && M > 2) return -22;                 // fp8 weights are a decode-only stream
    // rows <= 8 stream the weights through the GEMV family, which plans its own kernel (gemv.hip::gemv_plan); 9..16 rows too where
    // that family takes them (gemv_rows_9_16_ok) -- a 128-row GEMM tile would be > 87 % padding there
    if (M <= 8 || gemv_rows_9_16_ok(M, K, lda, ldw, norm_w != nullptr, wscale != nullptr, epi)) {
        GemvArgs g{A, W, norm_w, bias, res, C, M, N, K, lda, ldw, ldres, ldc, eps, epi, wscale};
        if (warm && M == 1 && !wscale) g.warm = *warm;
        return gemv_profiled(set_bytes(wscale ? WeightSet::Fp8 : WeightSet::Bf16, N, K), s, [&] { return launch_gemv(g, s); });
    }
    if (norm_w) return -22;
    GemmArgs g{A, W, bias, res, C, M, N, K, lda, ldw, ldres, ldc, epi, ConvGeom{0, 0, 0, 0, 0, 0}, nullptr, 0, 0};
    g.partial = splitk; g.partial_floats = splitk_floats;
    return launch_gemm(g, s);
}
// ---- The one rule that picks a projection's kernel from an engine's weight mode (emu_weight_mode: what the setters took), in two pure
// functions on integers -- no HIP call, no model.  emu_llama_projection_kernel is both; include/emu_hip.h states them in full.
constexpr bool fp8_prefill(const emu_weight_mode& md) { return md.fp8 == 2 || md.fp8 == 4 || md.fp8 == 6; }   // W8A8 GEMMs on
constexpr bool quantised(const emu_weight_mode& md) { return md.fp8 != 0 || md.fp4 != 0; }                    // an fp8 / fp4 stream on
// The call-level rule: the kernel a call of `rows` rows is planned around, from the mode and the shard's reduction widths (fp8 modes
// 3 / 4 = 1 / 2 plus the few-row stream, 5 / 6 = 3 / 4 plus the W8A16 GEMM; above 2 rows fp8 needs whole k stages / tiles, else bf16;
// the fp8_all switch puts mode 5's calls of 65 rows and more on the W8A16 GEMM's third form, mode 6 keeps the W8A8 GEMMs there)
WeightKernel call_kernel(const emu_weight_mode& md, int rows, int H, int HD, int Fl) {
    const auto whole = [&](int k) { return !(H & (k - 1)) && !(HD & (k - 1)) && !(Fl & (k - 1)); };
    if (serves(WeightKernel::Fp4Rows, rows)) return md.fp4 >= 1 ? WeightKernel::Fp4Rows : md.fp8 >= 1 ? WeightKernel::Fp8Rows : WeightKernel::Bf16;
    if (serves(WeightKernel::Fp4Thin, rows)) return md.fp4 >= 2 ? WeightKernel::Fp4Thin : md.fp8 >= 3 && whole(256) ? WeightKernel::Fp8Thin : WeightKernel::Bf16;
    if (md.fp4 == 3) return WeightKernel::Fp4Gemm;
    if (md.fp8 >= 5 && serves(WeightKernel::Fp8Stream, rows) && whole(256)) return WeightKernel::Fp8Stream;
    if (md.fp8 == 5 && md.fp8_all && serves(WeightKernel::Fp8Tile, rows) && whole(256)) return WeightKernel::Fp8Tile;
    return fp8_prefill(md) && whole(128) ? WeightKernel::Fp8Gemm : WeightKernel::Bf16;
}
// The matrix-level rule: the kernel that launches for ONE matrix at one call site, from the call-level answer k and the facts q
// (of the call only `rows` is read), and into q.norm_in_stream whether the RMSNorm rides in the weight stream.  A layer projection
// fuses the norm where its plan asks (q.norm) and runs the W8A8 GEMM as bf16 without an fp8 copy.  The head decides the norm itself; it
// has no W8A8 GEMM (under the fp8_all switch the W8A16 tile runs in its place where the head has an fp8 copy and K is in whole stages),
// its fp8 copy is optional, and the 3..16-row byte streams need the workspace for the normalised rows (all: bf16; MXFP4, and fp8 under
// fp8_all, only while there are bf16 weights).  Then a matrix left on bf16 streams its 13-bit packed set instead -- same bits, 13/16 of the bytes
// -- at one row unless a fused-layer / decode-tail / L2-warm mode inhibits it, at 4..16 rows under the wide switch and no fused norm.
WeightKernel matrix_kernel(WeightKernel k, emu_projection& q) {
    const bool released8 = q.mode.bf16_released && q.mode.fp8_all;       // (only the fp8 set is left: nothing to fall back to)
    const bool no_copy = needs_fp8(k) && !q.has_fp8;
    const bool no_ws = ((k == WeightKernel::Fp8Thin && !released8) || (k == WeightKernel::Fp4Thin && !q.mode.bf16_released)) && !q.ws_fits;
    if (k == WeightKernel::Fp8Gemm && q.head && q.mode.fp8_all && q.has_fp8 && serves(WeightKernel::Fp8Tile, q.rows) && !(q.K & 255)) k = WeightKernel::Fp8Tile;
    else if (k == WeightKernel::Fp8Gemm ? q.head || !q.has_fp8 : q.head && (no_copy || no_ws)) k = WeightKernel::Bf16;
    const bool fused = q.head ? norm_rides(k) || (k == WeightKernel::Bf16 && (q.rows == 1 || (q.rows <= 8 && !q.ws_fits))) : q.norm != 0;
    q.norm_in_stream = fused;
    const int set_rows = q.set_n == q.N && q.set_k == q.K ? q.pack_rows : 0;
    if (k != WeightKernel::Bf16 || !q.mode.pack || set_rows <= 0) return k;
    GemvShape sh = gemv_one_row_shape(q.N, q.K, fused, q.epi);
    if (serves(WeightKernel::Bf16Pack, q.rows))
        return !q.fused_mode && !q.tail_mode && !q.warm_mask && gemv_pack_rows(gemv_plan(sh, q.tune), sh) == set_rows ? WeightKernel::Bf16Pack : k;
    if (fused || !q.mode.pack_wide || !serves(WeightKernel::Bf16PackThin, q.rows)) return k;       // (the twin takes no norm: KERNEL_FACTS)
    sh.M = q.rows;
    return gemv_pack_thin_plan(sh, set_rows, q.tune).status ? k : WeightKernel::Bf16PackThin;
}
// out = epi(x W^T [+ bias] [+ res]) from a weight record through the kernel k names: g is the launch block but for the weight
// pointers, which come from w (ldw in elements of the set k reads).  Every stream runs under the GEMV profiler at its set's price.
// Refused (-22): a set the record does not hold, a row count outside the kernel's range, Fp8Gemm (it needs the caller's quantised rows:
// linear_q8), and whatever the launcher behind the kernel refuses (shape -> plan -> pointer checks -> launch).  pack_wide: the engine's
// few-row switch (emu_llama_use_bf16_pack_wide); below 2, Bf16PackThin over a 12-bit set is refused.
int linear_w(WeightKernel k, const Weights& w, GemvArgs g, hipStream_t s, float* splitk = nullptr, size_t splitk_floats = 0, int pack_wide = 0) {
    const WeightSet set = facts(k).set;
    if (k == WeightKernel::Fp8Gemm || !holds(w, set) || !serves(k, g.M)) return -22;
    if (k == WeightKernel::Bf16 || k == WeightKernel::Fp8Rows)       // stream or GEMM by the rows, priced where it streams (linear)
        return linear(g.x, set == WeightSet::Fp8 ? B(w.W8) : w.W, g.bias, g.res, g.norm_w, g.out, g.M, g.N, g.K, g.ldx, g.ldw, g.ldres, g.ldo, g.eps,
                      g.epi, s, set == WeightSet::Fp8 ? w.s8 : nullptr, splitk, splitk_floats, &g.warm);
    const double bytes = set_bytes(set, g.N, g.K, w.pk.rows, w.pk.patch != nullptr);
    if (set == WeightSet::Fp8) {
        g.W = B(w.W8); g.wscale = w.s8;
        return gemv_profiled(bytes, s, [&] {
            return k == WeightKernel::Fp8Thin ? launch_gemv_thin_stream(g, s) : k == WeightKernel::Fp8Tile ? launch_gemm_fp8t_stream(g, s) : launch_gemm_fp8w_stream(g, s);
        });
    }
    if (set == WeightSet::Pack) {                    // the packed twins of the planned bf16 forms
        if (g.N != w.pkN || g.K != w.pkK || g.ldw != g.K) return -22;
        g.W = w.W;
        if (k == WeightKernel::Bf16PackThin) {
            if (w.pk.patch && pack_wide < 2) return -22;             // (a 12-bit set goes to its twin under switch value 2 only)
            const GemvPlan p = gemv_pack_thin_plan(gemv_shape_of(g), w.pk.rows, emu_gemm_tune_get());
            return p.status ? -22 : gemv_profiled(bytes, s, [&] { return launch_gemv_pack_thin(g, w.pk, p, s); });
        }
        const GemvShape sh = gemv_one_row_shape(g.N, g.K, g.norm_w != nullptr, g.epi);
        const GemvPlan p = gemv_plan(sh, emu_gemm_tune_get());
        return gemv_pack_rows(p, sh) != w.pk.rows ? -22 : gemv_profiled(bytes, s, [&] { return launch_gemv_pack(g, w.pk, p.form, s); });
    }
    g.W = B(w.W4); g.w4scale = w.s4;
    if (k == WeightKernel::Fp4Rows) return g.K & 31 ? -22 : gemv_profiled(bytes, s, [&] { return launch_gemv(g, s); });
    return gemv_profiled(bytes, s, [&] { return k == WeightKernel::Fp4Thin ? launch_gemv_thin_stream(g, s) : launch_gemm_fp4(g, s); });
}
// linear_w's launch block for a packed [N, K] matrix of the engines (scale rows at fp4_scale_stride(K)), no bias; norm_w: the fused RMSNorm or null
GemvArgs packed(WeightKernel k, const bf16_t* x, int ldx, const bf16_t* norm_w, float eps, const bf16_t* res, int ldres, bf16_t* out, int ldo, int M, int N, int K, int epi) {
    return {x, nullptr, norm_w, nullptr, res, out, M, N, K, ldx, K / set_kdiv(facts(k).set), ldres, ldo, norm_w ? eps : 0.f, epi, nullptr, nullptr, fp4_scale_stride(K)};
}
// the merged o_proj of a short shard (gemv_merge.hip) under the same GEMV launch profiler as linear()
int gemv_merge_profiled(const GemvMergeArgs& g, hipStream_t s) {
    return gemv_profiled(set_bytes(WeightSet::Bf16, g.N, g.K), s, [&] { return launch_gemv_merge(g, s); });
}
// the wait bound and loader waves of a persistent-engine launch (decode_engine.hip): 2 s and the kernel's default, unless the tool
// switches EMU_ENGINE_TIMEOUT_MS / EMU_ENGINE_LOADERS (tools/README.md) say otherwise
void engine_tool_switches(EngArgs& a) {
    a.limit_ticks = 200000000LL;
    if (const char* e = getenv("EMU_ENGINE_TIMEOUT_MS")) { const long ms = atol(e); if (ms > 0) a.limit_ticks = ms * 100000LL; }
    if (const char* e = getenv("EMU_ENGINE_LOADERS")) a.nload = atoi(e);
}
// tests: the plan the C-ABI primitives emu_linear_bf16 / emu_decode_fused_bf16 attach to their launch (emu_l2_warm_test_plan)
WarmPlan g_test_warm;
static_assert(sizeof(emu_warm_plan) == sizeof(WarmPlan) && offsetof(emu_warm_plan, xcds) == offsetof(WarmPlan, xcds) &&
              offsetof(emu_warm_plan, block_bytes) == offsetof(WarmPlan, block_bytes), "emu_warm_plan mirrors WarmPlan");
}  // namespace

int emu_ctx_fail(emu_ctx* c, int code, const char* what) { return fail(c, code, what); }

bool emu_prof_on() { return g_lprof.on; }
void emu_prof_begin(hipStream_t s) {
    g_lprof.cur_a = nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;             // eager launches only: no events inside a stream capture
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return; }
    if (g_lprof.used == g_lprof.pool.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { g_lprof.cur_a = nullptr; return; }
        g_lprof.pool.emplace_back(a, b);
    }
    g_lprof.cur_a = g_lprof.pool[g_lprof.used].first;
    g_lprof.cur_b = g_lprof.pool[g_lprof.used].second;
    ++g_lprof.used;
    (void)hipEventRecord(g_lprof.cur_a, s);
}
void emu_prof_drop() {                                   // the launch between begin and end did not happen (-95 / -22): forget the pair
    if (g_lprof.cur_a && g_lprof.used) --g_lprof.used;
    g_lprof.cur_a = nullptr;
}
void emu_prof_end(hipStream_t s, const char* klass, int M, int N, int K, int tag, double flops) {
    if (!g_lprof.cur_a) return;
    (void)hipEventRecord(g_lprof.cur_b, s);
    g_lprof.recs.push_back({g_lprof.cur_a, g_lprof.cur_b, klass, M, N, K, tag, flops});
    g_lprof.cur_a = nullptr;
}

extern "C" {

int emu_version(void) { return 6; }      // ABI version: emu_amd/_lib.py::ABI_VERSION must match
int emu_llama_projection_kernel(emu_projection* q) {
    if (!q || q->mode.fp8 < 0 || q->mode.fp8 > 6 || q->mode.fp4 < 0 || q->mode.fp4 > 3 || (q->mode.fp8 && q->mode.fp4) || q->rows < 1 ||
        q->mode.fp8_all < 0 || q->mode.fp8_all > 1 || (q->mode.fp8_all && q->mode.fp8 < 5) ||
        q->hidden < 1 || q->heads_dim_local < 1 || q->ffn_local < 1 || q->N < 1 || q->K < 1 || q->pack_rows < 0 || q->warm_mask < 0)
        return -22;
    return (int)matrix_kernel(call_kernel(q->mode, q->rows, q->hidden, q->heads_dim_local, q->ffn_local), *q);
}
int emu_llama_weight_kernel(int fp8_mode, int fp4_mode, int rows, int hidden, int heads_dim_local, int ffn_local) {
    return (int)call_kernel(emu_weight_mode{fp8_mode, fp4_mode, 0, 0, 0, 0}, rows, hidden, heads_dim_local, ffn_local);
}
// the two older hooks: the matrix-level rule at a layer projection with an fp8 copy -- the wide switch off; the one-row stream inhibited
int emu_llama_pack_kernel(int kernel, int rows, int pack_rows, int pack_on, int fused_mode, int tail_mode, int warm_mask, int N, int K,
                          int norm, int epi, int tune) {
    emu_projection q{{0, 0, pack_on, 0, 0, 0}, rows, 0, 0, 0, N, K, norm, epi, 1, pack_rows, N, K, fused_mode, tail_mode, warm_mask, tune, 0, 0, 0};
    return kernel < 0 || kernel > (int)WeightKernel::Fp8Thin ? -22 : (int)matrix_kernel((WeightKernel)kernel, q);
}
int emu_llama_pack_thin_kernel(int kernel, int rows, int pack_rows, int set_n, int set_k, int pack_on, int wide_on, int N, int K, int norm,
                               int epi, int tune) {
    emu_projection q{{0, 0, pack_on, wide_on, 0, 0}, rows, 0, 0, 0, N, K, norm, epi, 1, pack_rows, set_n, set_k, 1, 0, 0, tune, 0, 0, 0};
    return kernel < 0 || kernel > (int)WeightKernel::Bf16PackThin ? -22 : (int)matrix_kernel((WeightKernel)kernel, q);
}
int emu_bf16_pack_rows(int N, int K, int norm, int epi, int tune) {
    if (N < 1 || K < 8) return 0;
    const GemvShape sh = gemv_one_row_shape(N, K, norm != 0, epi);
    return gemv_pack_rows(gemv_plan(sh, tune), sh);
}
int emu_bf16_pack(const void* w_bf16, int ldw, int N, int K, int rows, void* lo, void* nib, void* sign, void* flags, int* hb_out,
                  emu_stream_t s) {
    return launch_bf16_pack(B(w_bf16), ldw, N, K, rows, lo, nib, sign, reinterpret_cast<uint32_t*>(flags), hb_out, S(s));
}
int emu_linear_bf16pack(const void* A, const void* W, const emu_bf16_pack_set* set, const void* res, const void* norm_w, void* C, int N,
                        int K, int form, float eps, int epi, emu_stream_t s) {
    if (!A || !W || !set || !C) return -22;
    GemvArgs g{B(A), B(W), B(norm_w), nullptr, B(res), B(C), 1, N, K, K, K, res ? N : 0, epi == EPI_SWIGLU ? N / 2 : N, eps, epi, nullptr};
    PackSet p;
    p.lo = set->lo; p.nib = set->nib; p.sign = set->sign; p.flags = reinterpret_cast<const uint32_t*>(set->flags); p.hb = set->hb; p.rows = set->rows;
    return launch_gemv_pack(g, p, form, S(s));
}
int emu_bf16_pack12(const void* w_bf16, int ldw, int N, int K, int rows, void* lo, void* nib, void* patch, void* flags, int* hb_out,
                    int* flagged_out, emu_stream_t s) {
    return launch_bf16_pack12(B(w_bf16), ldw, N, K, rows, lo, nib, patch, reinterpret_cast<uint32_t*>(flags), hb_out, flagged_out, S(s));
}
int emu_linear_bf16pack12(const void* A, const void* W, const emu_bf16_pack12_set* set, const void* res, const void* norm_w, void* C,
                          int N, int K, int form, float eps, int epi, emu_stream_t s) {
    if (!A || !W || !set || !C || !set->patch) return -22;
    GemvArgs g{B(A), B(W), B(norm_w), nullptr, B(res), B(C), 1, N, K, K, K, res ? N : 0, epi == EPI_SWIGLU ? N / 2 : N, eps, epi, nullptr};
    PackSet p;
    p.lo = set->lo; p.nib = set->nib; p.patch = reinterpret_cast<const uint32_t*>(set->patch); p.flags = reinterpret_cast<const uint32_t*>(set->flags);
    p.hb = set->hb; p.rows = set->rows;
    return launch_gemv_pack(g, p, form, S(s));
}
int emu_linear_bf16pack_thin(const void* A, const void* W, const emu_bf16_pack_set* set, const void* res, void* C, int M, int N, int K,
                             int epi, emu_stream_t s) {
    if (!A || !W || !set || !C) return -22;
    GemvArgs g{B(A), B(W), nullptr, nullptr, B(res), B(C), M, N, K, K, K, res ? N : 0, epi == EPI_SWIGLU ? N / 2 : N, 0.f, epi, nullptr};
    PackSet p;
    p.lo = set->lo; p.nib = set->nib; p.sign = set->sign; p.flags = reinterpret_cast<const uint32_t*>(set->flags); p.hb = set->hb; p.rows = set->rows;
    const GemvPlan pl = gemv_pack_thin_plan(gemv_shape_of(g), p.rows, emu_gemm_tune_get());
    return pl.status ? -22 : launch_gemv_pack_thin(g, p, pl, S(s));
}
int emu_linear_bf16pack12_thin(const void* A, const void* W, const emu_bf16_pack12_set* set, const void* res, void* C, int M, int N, int K,
                               int epi, emu_stream_t s) {
    if (!A || !W || !set || !C || !set->patch) return -22;
    GemvArgs g{B(A), B(W), nullptr, nullptr, B(res), B(C), M, N, K, K, K, res ? N : 0, epi == EPI_SWIGLU ? N / 2 : N, 0.f, epi, nullptr};
    PackSet p;
    p.lo = set->lo; p.nib = set->nib; p.patch = reinterpret_cast<const uint32_t*>(set->patch); p.flags = reinterpret_cast<const uint32_t*>(set->flags);
    p.hb = set->hb; p.rows = set->rows;
    const GemvPlan pl = gemv_pack_thin_plan(gemv_shape_of(g), p.rows, emu_gemm_tune_get());
    return pl.status ? -22 : launch_gemv_pack_thin(g, p, pl, S(s));
}

void emu_set_splitk_scratch(void* ptr, size_t bytes) { emu_gemm_set_splitk_scratch(reinterpret_cast<float*>(ptr), bytes / sizeof(float)); }
void emu_gemm_force_config(int cfg) { emu_gemm_force_config_set(cfg); }
void emu_gemm_tune(int mask) { emu_gemm_tune_set(mask); }
void emu_gemm_trace(void* buf) { emu_gemm_trace_set(reinterpret_cast<unsigned long long*>(buf)); }
void emu_gemm_trace_nth(long n) { emu_gemm_trace_select(n); }
int emu_gemm_trace_built(void) {
#ifdef EMU_TRACE
    return 1;
#else
    return 0;
#endif
}

int emu_profile_launches(int enable) {
    g_lprof.on = enable != 0;
    g_lprof.recs.clear();
    g_lprof.used = 0;
    return 0;
}
int emu_profile_launches_read(emu_prof_row* rows, int cap) {
    int n = 0;
    for (const auto& r : g_lprof.recs) {
        if (hipEventSynchronize(r.b) != hipSuccess) return -5;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return -5;
        int i = 0;
        for (; i < n; ++i)
            if (!strcmp(rows[i].klass, r.klass) && rows[i].M == r.M && rows[i].N == r.N && rows[i].K == r.K && rows[i].tag == r.tag) break;
        if (i == n) {
            if (n == cap) continue;
            memset(&rows[n], 0, sizeof rows[n]);
            strncpy(rows[n].klass, r.klass, sizeof rows[n].klass - 1);
            rows[n].M = r.M; rows[n].N = r.N; rows[n].K = r.K; rows[n].tag = r.tag;
            ++n;
        }
        rows[i].launches += 1; rows[i].ms += ms; rows[i].flops += r.flops;
    }
    return n;
}

int emu_profile_gemv(int enable) {
    g_prof.on = enable != 0;
    g_prof.used = 0;
    g_prof.bytes = 0.0;
    return 0;
}

int emu_profile_gemv_read(double* total_ms, double* weight_bytes, long* launches) {
    double t = 0.0;
    for (size_t i = 0; i < g_prof.used; ++i) {
        hipError_t e = hipEventSynchronize(g_prof.ev[i].second);
        if (e != hipSuccess) return (int)e;
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, g_prof.ev[i].first, g_prof.ev[i].second);
        if (e != hipSuccess) return (int)e;
        t += ms;
    }
    if (total_ms) *total_ms = t;
    if (weight_bytes) *weight_bytes = g_prof.bytes;
    if (launches) *launches = (long)g_prof.used;
    return 0;
}

int emu_ctx_create(int device, int tp_rank, int tp_size, emu_ctx** out) {
    if (!out || tp_size < 1 || tp_rank < 0 || tp_rank >= tp_size) return -22;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || device < 0 || device >= n) return e != hipSuccess ? (int)e : -19;
    emu_ctx* c = new emu_ctx();
    c->device = device; c->tp_rank = tp_rank; c->tp_size = tp_size;
    if (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) { (void)hipGetLastError(); c->ncu = 0; }
    *out = c;
    return 0;
}

void emu_ctx_destroy(emu_ctx* ctx) {
    if (!ctx) return;
    if (ctx->comm) ncclCommDestroy(ctx->comm);
    emu_p2p_destroy(ctx->p2p);
    for (hipEvent_t e : ctx->ar_ev) if (e) (void)hipEventDestroy(e);
    if (ctx->lane_stream) (void)hipStreamDestroy(ctx->lane_stream);
    delete ctx;
}

const char* emu_last_error(const emu_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int emu_tp_unique_id(void* out128) {
    static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id is 128 bytes");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return 1000 + (int)r;
    memcpy(out128, &id, sizeof id);
    return 0;
}

int emu_tp_init(emu_ctx* ctx, const void* id128) {
    if (!ctx) return -22;
    if (ctx->comm) return 0;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, (int)e, "hipSetDevice");
    ncclResult_t r = ncclCommInitRank(&ctx->comm, ctx->tp_size, id, ctx->tp_rank);
    if (r != ncclSuccess) { ctx->comm = nullptr; return fail(ctx, 1000 + (int)r, "ncclCommInitRank"); }
    return 0;
}

int emu_tp_p2p_create(emu_ctx* ctx, void* handle64_out) {
    if (!ctx || !handle64_out) return -22;
    if (ctx->p2p) return fail(ctx, -17, "emu_tp_p2p_create: already created");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, (int)e, "hipSetDevice");
    ctx->p2p = emu_p2p_create(ctx->tp_rank, ctx->tp_size, handle64_out);
    return ctx->p2p ? 0 : fail(ctx, -12, "emu_tp_p2p_create: comm block allocation / IPC export failed");
}

int emu_tp_p2p_open(emu_ctx* ctx, const void* handles, int timeout_ms) {
    if (!ctx || !ctx->p2p) return -22;
    hipError_t e = hipSetDevice(ctx->device);              // the peer blocks are mapped for this context's device
    if (e != hipSuccess) return fail(ctx, (int)e, "hipSetDevice");
    emu_p2p_set_timeout_ms(ctx->p2p, timeout_ms);
    int st = emu_p2p_open(ctx->p2p, handles);
    return st == 0 ? 0 : fail(ctx, st, "hipIpcOpenMemHandle");
}

int emu_tp_p2p_allreduce_bf16(emu_ctx* ctx, void* buf, size_t n, emu_stream_t s) {
    if (!ctx || !ctx->p2p) return -22;
    int st = emu_p2p_allreduce(ctx->p2p, reinterpret_cast<bf16_t*>(buf), n, S(s));
    return st == 0 ? 0 : fail(ctx, st, "emu_p2p_allreduce");
}

int emu_tp_p2p_enable(emu_ctx* ctx, int on) {
    if (!ctx || (on && !ctx->p2p)) return -22;
    ctx->p2p_on = on != 0;
    return 0;
}

int emu_tp_p2p_set_fenced(emu_ctx* ctx, int fenced) {
    if (!ctx || !ctx->p2p) return -22;
    emu_p2p_set_fenced(ctx->p2p, fenced);
    return 0;
}
int emu_tp_p2p_fenced(const emu_ctx* ctx) { return ctx && ctx->p2p ? emu_p2p_fenced(ctx->p2p) : -1; }
unsigned int emu_tp_p2p_giveups(void) { return emu_p2p_giveups_read(); }

int emu_allreduce_bf16(emu_ctx* ctx, void* buf, size_t n, emu_stream_t s) {
    if (!ctx) return -22;
    // small messages (decode: 13 KB) take the one-shot P2P path once the host has enabled it; without a RCCL communicator
    // (two ranks on one GPU in the tests) everything does, in slot-sized chunks
    if (ctx->p2p_on && (n * sizeof(bf16_t) <= EMU_P2P_SLOT_BYTES || !ctx->comm)) {
        int st = emu_p2p_allreduce(ctx->p2p, reinterpret_cast<bf16_t*>(buf), n, S(s));
        return st == 0 ? 0 : fail(ctx, st, "emu_p2p_allreduce");
    }
    if (!ctx->comm) {
        if (ctx->tp_size == 1) return 0;
        return fail(ctx, -107, "emu_allreduce_bf16: communicator not initialised (emu_tp_init)");
    }
    ncclResult_t r = ncclAllReduce(buf, buf, n, ncclBfloat16, ncclSum, ctx->comm, S(s));
    return r == ncclSuccess ? 0 : fail(ctx, 1000 + (int)r, "ncclAllReduce");
}

// ---------------------------------------------------------------------------------------------- primitives
int emu_linear_bf16(const void* A, const void* W, const void* bias, const void* res, const void* norm_w, void* C,
                    int M, int N, int K, int lda, int ldw, int ldres, int ldc, float eps, int epi, emu_stream_t s) {
    return linear(B(A), B(W), B(bias), B(res), B(norm_w), B(C), M, N, K, lda, ldw, ldres, ldc, eps, epi, S(s), nullptr, nullptr, 0,
                  g_test_warm.ntouch ? &g_test_warm : nullptr);
}
// ---- L2 warming (l2_warm.h): the plan arithmetic for the CPU test, and a test hook that attaches a plan to the primitives
int emu_l2_warm_plan_make(const void* base, long twin, unsigned rows, unsigned row_bytes, unsigned used_bytes, unsigned long long nrows,
                          unsigned gx, unsigned groups, unsigned pred_wgs, int extra, unsigned lanes, unsigned long long budget_bytes,
                          int shape, emu_warm_plan* out) {
    if (!out) return -22;
    WarmSucc su;
    su.base = base; su.twin = twin; su.rows = rows; su.row_bytes = row_bytes; su.used_bytes = used_bytes; su.nrows = nrows;
    su.gx = gx; su.groups = groups ? groups : 1;
    const WarmPlan p = make_warm_plan(su, pred_wgs, extra != 0, lanes, budget_bytes, shape);
    memcpy(out, &p, sizeof p);
    return 0;
}
long emu_l2_warm_enumerate(const emu_warm_plan* plan, unsigned wg, long long* offsets, long cap) {
    if (!plan) return -22;
    WarmPlan p;
    memcpy(&p, plan, sizeof p);
    long n = 0;
    const uint32_t trips = warm_trips(p, wg);
    for (uint32_t i = 0; i < trips; ++i)
        for (uint32_t t = 0; t < p.lanes; ++t) {
            const int64_t off = warm_line(p, wg, t, i);
            if (off < 0) continue;
            if (offsets && n < cap) offsets[n] = off;
            ++n;
        }
    return n;
}
int emu_gemv_geometry_query(int N, int K, int norm, int epi, int out[4]) {
    if (!out || N < 1 || K < 8) return -22;
    const GemvGeom g = emu_gemv_geometry(N, K, norm != 0, epi);
    out[0] = g.form; out[1] = g.rows; out[2] = emu_gemv_rows_per_block(N, K, norm != 0); out[3] = emu_gemv_partition(N, K, norm != 0, epi);
    return 0;
}
void emu_l2_warm_test_plan(const emu_warm_plan* plan) {
    g_test_warm = WarmPlan{};
    if (plan) memcpy(&g_test_warm, plan, sizeof g_test_warm);
}
int emu_linear_fp8w_bf16(const void* A, const void* W8, const float* wscale, const void* bias, const void* res,
                         const void* norm_w, void* C, int M, int N, int K, int lda, int ldw, int ldres, int ldc, float eps,
                         int epi, emu_stream_t s) {
    if (!wscale) return -22;
    return linear(B(A), B(W8), B(bias), B(res), B(norm_w), B(C), M, N, K, lda, ldw, ldres, ldc, eps, epi, S(s), wscale);
}
int emu_linear_fp8w_thin_bf16(const void* A, const void* W8, const float* wscale, const void* bias, const void* res, void* C, int M, int N,
                              int K, int lda, int ldw, int ldres, int ldc, int epi, emu_stream_t s) {
    if (!A || !W8 || !wscale || !C) return -22;
    return linear_w(WeightKernel::Fp8Thin, {nullptr, U8(W8), wscale},
                    {B(A), nullptr, nullptr, B(bias), B(res), B(C), M, N, K, lda, ldw, ldres, ldc, 0.f, epi}, S(s));
}
int emu_linear_fp8w_gemm_bf16(const void* A, const void* W8, const float* wscale, const void* bias, const void* res, void* C, int M, int N,
                              int K, int lda, int ldw, int ldres, int ldc, int epi, emu_stream_t s) {
    if (!A || !W8 || !wscale || !C) return -22;
    return linear_w(WeightKernel::Fp8Stream, {nullptr, U8(W8), wscale},
                    {B(A), nullptr, nullptr, B(bias), B(res), B(C), M, N, K, lda, ldw, ldres, ldc, 0.f, epi}, S(s));
}
int emu_linear_fp8w_tile_bf16(const void* A, const void* W8, const float* wscale, const void* bias, const void* res, void* C, int M, int N,
                              int K, int lda, int ldw, int ldres, int ldc, int epi, emu_stream_t s) {
    if (!A || !W8 || !wscale || !C) return -22;
    return linear_w(WeightKernel::Fp8Tile, {nullptr, U8(W8), wscale},
                    {B(A), nullptr, nullptr, B(bias), B(res), B(C), M, N, K, lda, ldw, ldres, ldc, 0.f, epi}, S(s));
}
// the four MXFP4 entry points name their kernel (the caller's matrix as a weight record, its arguments as the launch block);
// linear_w refuses a row count outside the kernel's range
static int linear_fp4w(WeightKernel k, const void* A, const void* W4, const void* scales, const void* bias, const void* res, const void* norm_w,
                       void* C, int M, int N, int K, int lda, int ldw, int lds, int ldres, int ldc, float eps, int epi, emu_stream_t s) {
    if (!A || !W4 || !scales || !C) return -22;
    return linear_w(k, {nullptr, nullptr, nullptr, U8(W4), U8(scales)},
                    {B(A), nullptr, B(norm_w), B(bias), B(res), B(C), M, N, K, lda, ldw, ldres, ldc, eps, epi, nullptr, nullptr, lds}, S(s));
}
int emu_linear_fp4w_bf16(const void* A, const void* W4, const void* scales, const void* bias, const void* res,
                         const void* norm_w, void* C, int M, int N, int K, int lda, int ldw, int lds, int ldres, int ldc, float eps,
                         int epi, emu_stream_t s) {
    if (M < 1 || K < 32) return -22;
    return linear_fp4w(WeightKernel::Fp4Rows, A, W4, scales, bias, res, norm_w, C, M, N, K, lda, ldw, lds, ldres, ldc, eps, epi, s);
}
int emu_linear_fp4w_mfma_bf16(const void* A, const void* W4, const void* scales, const void* bias, const void* res, void* C, int M, int N,
                              int K, int lda, int ldw, int lds, int ldres, int ldc, int epi, emu_stream_t s) {
    return linear_fp4w(M <= 16 ? WeightKernel::Fp4Thin : WeightKernel::Fp4Gemm, A, W4, scales, bias, res, nullptr, C, M, N, K, lda, ldw, lds, ldres, ldc, 0.f, epi, s);
}
// the two older entry points keep K in whole stages (K % 256 == 0), refused here: the launchers behind them take a partial last stage
int emu_linear_fp4w_thin_bf16(const void* A, const void* W4, const void* scales, const void* bias, const void* res, void* C, int M, int N,
                              int K, int lda, int ldw, int lds, int ldres, int ldc, int epi, emu_stream_t s) {
    return K & 255 ? -22 : linear_fp4w(WeightKernel::Fp4Thin, A, W4, scales, bias, res, nullptr, C, M, N, K, lda, ldw, lds, ldres, ldc, 0.f, epi, s);
}
int emu_linear_fp4w_gemm_bf16(const void* A, const void* W4, const void* scales, const void* bias, const void* res, void* C, int M, int N,
                              int K, int lda, int ldw, int lds, int ldres, int ldc, int epi, emu_stream_t s) {
    return K & 255 ? -22 : linear_fp4w(WeightKernel::Fp4Gemm, A, W4, scales, bias, res, nullptr, C, M, N, K, lda, ldw, lds, ldres, ldc, 0.f, epi, s);
}
int emu_quantize_mxfp4_rows(const void* w, int ldw, void* q, int ldq, void* scales, int lds, int N, int K, emu_stream_t s) {
    if (!w || !q || !scales) return -22;
    return launch_quant_mxfp4_rows(B(w), ldw, reinterpret_cast<uint8_t*>(q), ldq, reinterpret_cast<uint8_t*>(scales), lds, N, K, S(s));
}
int emu_linear_fp8_bf16(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias,
                        const void* res, void* C, int M, int N, int K, int lda, int ldw, int ldres, int ldc, int epi,
                        emu_stream_t s) {
    if (!A8 || !W8 || !a_scale || !w_scale || !C) return -22;
    GemmArgs g{B(A8), B(W8), B(bias), B(res), B(C), M, N, K, lda, ldw, ldres, ldc, epi, ConvGeom{0, 0, 0, 0, 0, 0}, nullptr, 0, 0};
    g.a_scale = a_scale; g.w_scale = w_scale;
    return launch_gemm_fp8(g, S(s));
}
int emu_linear_fused_bf16(const void* A, const void* W, const void* bias, const void* res, void* C, int M, int N, int K,
                          int lda, int ldw, int ldres, int ldc, int epi, const emu_linear_fx* fx, emu_stream_t s) {
    if (!A || !W || !C || M <= 8) return -22;
    GemmArgs g{B(A), B(W), B(bias), B(res), B(C), M, N, K, lda, ldw, ldres, ldc, epi, ConvGeom{0, 0, 0, 0, 0, 0}, nullptr, 0, 0};
    if (fx) {
        g.row_stats_out = fx->row_stats_out;
        g.ln_c = fx->ln_c; g.ln_d = fx->ln_d; g.ln_stats = fx->ln_stats; g.ln_slots = fx->ln_slots; g.ln_eps = fx->ln_eps;
        g.vt_out = B(fx->vt_out); g.vt_col0 = fx->vt_col0; g.vt_s = fx->vt_s; g.vt_spad = fx->vt_spad;
        g.cross_k = B(fx->cross_k); g.cross_vt = B(fx->cross_vt); g.cross_ldk = fx->cross_ldk; g.cross_n = fx->cross_n;
        g.cross_npad = fx->cross_npad; g.cross_rows = fx->cross_rows; g.cross_scale = fx->cross_scale;
    }
    return launch_gemm(g, S(s));
}
int emu_quantize_fp8_rows(const void* w, int ldw, void* q, int ldq, float* scale, int N, int K, emu_stream_t s) {
    if (!w || !q || !scale) return -22;
    return launch_quant_fp8_rows(B(w), ldw, reinterpret_cast<uint8_t*>(q), ldq, scale, N, K, S(s));
}
int emu_rmsnorm_bf16(const void* x, const void* w, void* y, int rows, int cols, int ldx, int ldy, float eps, emu_stream_t s) {
    return launch_rmsnorm(B(x), B(w), B(y), rows, cols, ldx, ldy, eps, S(s));
}
int emu_layernorm_bf16(const void* x, const void* w, const void* b, const void* res, void* y, int rows, int cols,
                       float eps, emu_stream_t s) {
    return launch_layernorm(B(x), B(w), B(b), B(res), B(y), rows, cols, eps, S(s));
}
int emu_layernorm_q8_bf16(const void* x, const void* w, const void* b, const void* res, void* y, void* q, float* scale, int rows,
                          int cols, float eps, emu_stream_t s) {
    if (!x || !w || !b || !q || !scale) return -22;
    return launch_layernorm_q8(B(x), B(w), B(b), B(res), reinterpret_cast<bf16_t*>(y), reinterpret_cast<uint8_t*>(q), scale, rows, cols,
                               eps, S(s));
}
static int chain_out_len(const emu_chain_op& o) { return o.epi == EPI_SWIGLU ? o.N / 2 : o.N; }
size_t emu_gemv_chain_granule_bytes(const emu_chain_op* ops, int nops) {
    size_t b = 0;
    for (int i = 0; ops && i + 1 < nops; ++i)
        if (ops[i + 1].x_from_prev) b += align_up((size_t)chain_out_len(ops[i]) * 4);
    return b;
}
int emu_gemv_chain_bf16(emu_ctx* ctx, const emu_chain_op* ops, int nops, void* granules, size_t granule_bytes, unsigned int* err,
                        emu_stream_t s_) {
    if (!ctx || !ops || nops < 1 || nops > ENG_MAX_OPS || !err) return -22;
    const size_t need = emu_gemv_chain_granule_bytes(ops, nops);
    if (need > granule_bytes || (need && !granules)) return fail(ctx, -12, "emu_gemv_chain_bf16: granule buffer too small");
    hipStream_t s = S(s_);
    EngArgs a{};
    a.nops = nops; a.err = err;
    engine_tool_switches(a);
    if (const char* e = getenv("EMU_ENGINE_DBG")) a.dbg = atoi(e);
    if (ctx->ncu < 1) return -5;
    a.ncu = ctx->ncu;
    char* gp = reinterpret_cast<char*>(granules);
    size_t off = 0;
    for (int i = 0; i < nops; ++i) {
        const emu_chain_op& c = ops[i];
        EngOp& o = a.op[i];
        o.W = B(c.W); o.N = c.N; o.K = c.K; o.gain = B(c.gain); o.eps = c.eps; o.epi = c.epi; o.res = B(c.res);
        o.vw = emu_gemv_partition(c.N, c.K, c.gain != nullptr, c.epi);
        o.x_src = c.x_from_prev ? 1 : 0;
        o.xg = B(c.x);
        if (c.x_from_prev) {
            if (i == 0 || chain_out_len(ops[i - 1]) != c.K) return fail(ctx, -22, "emu_gemv_chain_bf16: op input is not the previous op's output");
            o.xgran = a.op[i - 1].ogran;
        }
        const bool to_next = i + 1 < nops && ops[i + 1].x_from_prev;
        o.out_dst = to_next ? 1 : 0;
        o.out = B(c.out);
        if (to_next) { o.ogran = reinterpret_cast<uint32_t*>(gp + off); off += align_up((size_t)chain_out_len(c) * 4); }
    }
    if (need && hipMemsetAsync(granules, 0, need, s) != hipSuccess) return fail(ctx, -5, "emu_gemv_chain_bf16: hipMemsetAsync");
    const int st = launch_decode_engine(a, s);
    return st == 0 || st == -95 ? st : fail(ctx, st, "emu_gemv_chain_bf16");
}
int emu_prefetch(const void* ptr, size_t bytes, int workgroups, emu_stream_t s) { return launch_prefetch(ptr, bytes, workgroups, S(s)); }
int emu_softmax_rows_bf16(void* x, const void* bias, int rows, int cols, int ld, int ld_bias, float scale, emu_stream_t s) {
    return launch_softmax_rows(B(x), B(bias), rows, cols, ld, ld_bias, scale, S(s));
}
int emu_embed_gather_bf16(const int32_t* ids, const void* table, void* out, int n_tok, int hidden, int vocab, emu_stream_t s) {
    return launch_embed_gather(ids, B(table), B(out), n_tok, hidden, vocab, S(s));
}
int emu_scatter_rows_bf16(const void* src, const int32_t* dst_rows, void* out, int n_rows, int hidden, emu_stream_t s) {
    return launch_scatter_rows(B(src), dst_rows, B(out), n_rows, hidden, S(s));
}
int emu_argmax_bf16(const void* logits, int ld, int rows, int vocab, int suppress_id, int32_t* out, emu_stream_t s) {
    return launch_argmax(B(logits), ld, rows, vocab, suppress_id, out, S(s));
}
int emu_sample_bf16(const void* logits, int ld, int rows, int vocab, const int32_t* hist, int hist_ld, int hist_rows,
                    const int32_t* step_dev, const float* uniforms, int uni_ld, int uni_rows, const emu_sample_params* params,
                    int32_t* unfinished, int32_t* out, float* probs_out, int ld_probs, emu_stream_t s) {
    return launch_sample(B(logits), ld, rows, vocab, hist, hist_ld, hist_rows, step_dev, uniforms, uni_ld, uni_rows, params, unfinished,
                         out, probs_out, ld_probs, nullptr, nullptr, 0, S(s));
}
int emu_sample_ngram_bf16(const void* logits, int ld, int rows, int vocab, const int32_t* hist, int hist_ld, int hist_rows,
                          const int32_t* step_dev, const float* uniforms, int uni_ld, int uni_rows, const emu_sample_params* params,
                          int32_t* unfinished, int32_t* out, float* probs_out, int ld_probs, int ngram, emu_stream_t s) {
    if (ngram < 0) return -22;
    return launch_sample(B(logits), ld, rows, vocab, hist, hist_ld, hist_rows, step_dev, uniforms, uni_ld, uni_rows, params, unfinished,
                         out, probs_out, ld_probs, nullptr, nullptr, ngram, S(s));
}
int emu_sample_trie_bf16(const void* logits, int ld, int rows, int vocab, const int32_t* hist, int hist_ld, int hist_rows,
                         const int32_t* step_dev, const float* uniforms, int uni_ld, int uni_rows, const emu_sample_params* params,
                         int32_t* unfinished, int32_t* out, float* probs_out, int ld_probs, const emu_token_trie* trie, int32_t* node,
                         emu_stream_t s) {
    if (!trie || !node) return -22;
    return launch_sample(B(logits), ld, rows, vocab, hist, hist_ld, hist_rows, step_dev, uniforms, uni_ld, uni_rows, params, unfinished,
                         out, probs_out, ld_probs, trie, node, 0, S(s));
}
int emu_token_logprob_bf16(const void* logits, int ld, int rows, int vocab, const int32_t* targets, int tgt_ld, const int32_t* step_dev,
                           const void* ref_logits, int ref_ld, float* lp, float* lse, int32_t* top1, float* kl, int32_t* agree,
                           int out_ld, emu_stream_t s) {
    return launch_token_logprob(B(logits), ld, rows, vocab, targets, tgt_ld, step_dev, 0, B(ref_logits), ref_ld, lp, lse, top1, kl, agree,
                                out_ld, nullptr, S(s));
}
int emu_patchify(const void* image, int image_is_f32, void* out, int Bn, int C, int HW, int patch, int Kpad, emu_stream_t s) {
    return launch_patchify(image, image_is_f32, B(out), Bn, C, HW, patch, Kpad, S(s));
}
size_t emu_image_resample_ws_bytes(int H, int W, int Sz) { return image_resample_ws_bytes(H, W, Sz); }
int emu_image_resample_norm(const uint8_t* src, long pitch, int H, int W, const int32_t* hcoef, const int32_t* hbounds, int hk,
                            const int32_t* vcoef, const int32_t* vbounds, int vk, int row0, int nrows, const float* lut, void* out,
                            int out_is_f32, int Sz, void* ws, size_t ws_bytes, emu_stream_t s) {
    ImageResampleArgs a{src, pitch, H, W, hcoef, hbounds, hk, vcoef, vbounds, vk, row0, nrows, lut, out, out_is_f32, Sz, ws, ws_bytes};
    return launch_image_resample_norm(a, S(s));
}
int emu_image_to_u8_nhwc(const void* x, uint8_t* out, int N, int C, int H, int W, emu_stream_t s) {
    return launch_image_to_u8(B(x), out, N, C, H, W, S(s));
}
int emu_vit_assemble_bf16(const void* patches, const void* cls, const void* pos, void* x, int Bn, int T, int C, emu_stream_t s) {
    return launch_vit_assemble(B(patches), B(cls), B(pos), B(x), Bn, T, C, S(s));
}
int emu_avgpool_tokens_bf16(const void* x, void* out, int Bn, int g, int C, int stride, emu_stream_t s) {
    return launch_avgpool_tokens(B(x), B(out), Bn, g, C, stride, S(s));
}
int emu_rope_kv_append_bf16(void* qkv, const void* cos, const void* sin, const int32_t* pos, const int32_t* slot,
                            void* kcache, void* vcache, int Bn, int T, int H, int D, int S_max, emu_stream_t s) {
    RopeKvArgs a{B(qkv), B(cos), B(sin), pos, slot, B(kcache), B(vcache), Bn, T, H, D, S_max};
    return launch_rope_kv(a, S(s));
}
int emu_transpose_v_bf16(const void* v, long v_sb, long v_sh, long v_ss, void* vt, int Bn, int H, int Sn, int D,
                         int S_pad, emu_stream_t s) {
    TransposeVArgs a{B(v), v_sb, v_sh, v_ss, B(vt), Bn, H, Sn, D, S_pad};
    return launch_transpose_v(a, S(s));
}
int emu_flash_attn_bf16(const void* q, long q_sb, long q_sh, long q_ss, const void* k, long k_sb, long k_sh, long k_ss,
                        const void* vt, void* o, long o_sb, long o_sh, long o_ss, const int32_t* kstart, int Bn, int H,
                        int Sq, int Sk, int Sk_pad, int D, int causal, float scale, emu_stream_t s) {
    FlashArgs a{B(q), q_sb, q_sh, q_ss, B(k), k_sb, k_sh, k_ss, B(vt), B(o), o_sb, o_sh, o_ss, kstart,
                Bn, H, Sq, Sk, Sk_pad, D, causal, scale};
    return launch_flash_attn(a, S(s));
}
int emu_flash_attn_prefix_bf16(const void* q, long q_sb, long q_sh, long q_ss, const void* kprefix, long kp_sh, long kp_ss,
                               const void* vtprefix, const void* k, long k_sb, long k_sh, long k_ss, const void* vt, void* o, long o_sb,
                               long o_sh, long o_ss, int kstart, int Bn, int H, int Sq, int P, int P_pad, int Sk, int Sk_pad, int D,
                               float scale, emu_stream_t s) {
    FlashPrefixArgs a{B(q), q_sb, q_sh, q_ss, B(kprefix), kp_sh, kp_ss, B(vtprefix), B(k), k_sb, k_sh, k_ss, B(vt),
                      B(o), o_sb, o_sh, o_ss, nullptr, kstart, Bn, H, Sq, P, P_pad, Sk, Sk_pad, D, scale};
    return launch_flash_attn_prefix(a, S(s));
}
size_t emu_decode_attn_ws_bytes(int Bn, int H, int D, int ctx_max) {
    return (size_t)Bn * H * decode_attn_nsplit(ctx_max) * (D + 2) * sizeof(float);
}
int emu_decode_attn_bf16(const void* q, long q_sb, long q_sh, const void* kcache, const void* vcache, void* o,
                         long o_sb, long o_sh, const int32_t* kstart, const int32_t* ctx_dev, int ctx, int ctx_max,
                         void* ws, int Bn, int H, int D, int S_max, float scale, emu_stream_t s) {
    DecodeAttnArgs a{B(q), q_sb, q_sh, B(kcache), B(vcache), B(o), o_sb, o_sh, kstart, ctx_dev,
                     reinterpret_cast<float*>(ws), Bn, H, D, S_max, ctx, ctx_max, scale};
    return launch_decode_attn(a, S(s));
}
size_t emu_decode_fused_ws_bytes(int Bn, int H, int D, int ctx_max) { return decode_fused_ws_floats(Bn, H, D, ctx_max) * sizeof(float); }
int emu_decode_fused_bf16(const void* qkv, const void* cos, const void* sin, const int32_t* pos, const int32_t* slot,
                          void* kcache, void* vcache, void* o, long o_sb, long o_sh, const int32_t* kstart, void* ws, int Bn,
                          int H, int D, int S_max, int ctx_max, float scale, int share_nb, int share_len, int32_t* arrive,
                          emu_stream_t s) {
    DecodeFusedArgs a{B(qkv), B(cos), B(sin), pos, slot, B(kcache), B(vcache), B(o), o_sb, o_sh, kstart,
                      reinterpret_cast<float*>(ws), Bn, H, D, S_max, ctx_max, scale, share_nb, share_len, arrive};
    a.warm = g_test_warm;                            // (emu_l2_warm_test_plan; the launch ignores a plan that does not fit it)
    return launch_decode_fused(a, S(s));
}
size_t emu_decode_chunk_ws_bytes(int Bn, int T, int H, int D, int ctx_max) { return decode_chunk_ws_floats(Bn, T, H, D, ctx_max) * sizeof(float); }
int emu_decode_chunk_bf16(const void* qkv, const void* cos, const void* sin, const int32_t* pos0, const int32_t* slot0, void* kcache,
                          void* vcache, void* o, long o_sb, long o_sh, const int32_t* kstart, void* ws, int Bn, int T, int H, int D,
                          int S_max, int ctx_max, float scale, emu_stream_t s) {
    if (!qkv || !cos || !sin || !pos0 || !slot0 || !kcache || !vcache || !o || !ws) return -22;
    DecodeChunkArgs a{B(qkv), B(cos), B(sin), pos0, slot0, B(kcache), B(vcache), B(o), o_sb, o_sh, kstart,
                      reinterpret_cast<float*>(ws), Bn, T, H, D, S_max, ctx_max, scale};
    return launch_decode_chunk(a, S(s));
}

}  // extern "C"

// =============================================================================================== LLaMA engine
struct emu_llama {
    emu_ctx* ctx;
    emu_llama_cfg cfg;
    // one weight record per matrix (emu_llama_set_layer / _fp8 / _fp4 fill its three sets).  A layer without fp8 weights runs bf16
    // under the fp8 prefill; emu_llama_use_fp4 checks that every layer and the head have the MXFP4 set.
    struct Layer { Weights qkv, o, gu, down; const bf16_t *ln1 = nullptr, *ln2 = nullptr; };
    std::vector<Layer> layers;
    Weights head;                  // lm_head: the fp8 / MXFP4 copies cover the same rows (quantised from the shard)
    // the weight mode as the setters took it (include/emu_hip.h), fp8 and fp4 never both; what it means for a projection is call_kernel's and
    // matrix_kernel's to say.  bf16_released (emu_llama_release_bf16; fp4 mode 3, or fp8 modes 5 / 6 with fp8_all, which it pins): the
    // records' bf16 pointers are null.
    emu_weight_mode mode{};
    // the kernel a call of `rows` rows is planned around, layers and head alike
    WeightKernel kernel_for(int rows) const { return call_kernel(mode, rows, cfg.hidden, cfg.heads_local * cfg.head_dim, cfg.ffn_local); }
    // matrix_kernel's facts for the [N, K] matrix W under `rows` rows at a layer projection; the head sets its own two on top
    emu_projection site(const Weights& W, int rows, int N, int K, bool norm, int epi, int tail_mode, int warm_mask) const {
        return {mode, rows, cfg.hidden, cfg.heads_local * cfg.head_dim, cfg.ffn_local, N, K, norm, epi, W.W8 != nullptr, W.pk.patch && rows > 1 && mode.pack_wide < 2 ? 0 : W.pk.rows, W.pkN, W.pkK,       // (a 12-bit set: the one-row streams only, below switch value 2)
                decode_fused, tail_mode, warm_mask, emu_gemm_tune_get(), 0, 0, 0};
    }
    const bf16_t *final_norm = nullptr, *embed = nullptr, *cos = nullptr, *sin = nullptr;
    // tensor parallelism: lm_head holds rows [head_row0, head_row0 + head_rows) of the vocabulary only (emu_llama_set_head_shard);
    // head_rows < 0: the whole matrix
    int head_row0 = 0, head_rows = -1;
    bf16_t *kcache = nullptr, *vcache = nullptr;
    int kv_batch = 0, s_max = 0;
    int kv_share_nb = 0, kv_share_len = 0;       // emu_llama_set_kv_share: beams of a prompt share its cache slots
    // emu_llama_set_kv_prefix: T > 1 rows attend prefix[kstart .. prefix_len) of these read-only caches [layer, 1, Hl, prefix_s_max, D]
    // plus their own slots of kcache / vcache (attention_prefix.hip); prefix_len = 0: off
    const bf16_t *kprefix = nullptr, *vprefix = nullptr;
    int prefix_s_max = 0, prefix_len = 0;
    int l0 = 0, l1 = -1;                         // emu_llama_set_layer_range: layers [l0, l1) run (l1 < 0: all)
    bool fuse_norm_on = false;                   // sticky: o_proj / down_proj K-slice sums apply the RMSNorm behind them (M > 16, no TP)
    bool prefill_fusion = false;                 // emu_llama_set_prefill_fusion: RoPE + KV append + V^T in the qkv GEMM's epilogue (one-shot: the next T > 1 forward consumes it)
    // decode attention without the combine launch (emu_llama_set_decode_tail, off by default): per (row, head) arrival counters of
    // the split workgroups (zero between launches; owned here: EMU_ARRIVE_INTS ints of device memory)
    int* arrive = nullptr;
    // L2 warming across the launch boundaries of the default one-row bf16 step (emu_llama_set_l2_warm; l2_warm.h)
    int l2_warm = EMU_L2_WARM_DEFAULT;
    long warm_launches = 0;                      // launches that carried a non-empty plan (tests)
    bool decode_tail = false;                    // measured 0.4 % SLOWER than the combine launch (profiles/r04_decode_tail_merge_ab.log): opt-in
    // whole decoder layers of a one-row step in one launch (decode_layer.hip; emu_llama_set_decode_fused)
    int decode_fused = 0;                        // 0: the launches above; 1: fused where the shape / mode allows; 2: + in-kernel all-reduce
    int dl_per_launch = 0;                       // layers per launch (0: all)
    DecodeLayerPtrs* dl_table = nullptr;         // device copy of the layers' weight pointers
    bool dl_dirty = true;
    int* dl_cnt = nullptr;                       // arrival counters of all layers (zeroed at the head of every fused forward)
    size_t dl_cnt_bytes = 0;
    unsigned* dl_err = nullptr;                  // give-up counter
    long dl_forwards = 0;                        // fused forwards issued (tests: the path under test is the one that ran)
    unsigned long long* dl_trace = nullptr;      // emu_llama_set_decode_trace (tools; -DEMU_TRACE twin library only)
    // mode 4: the persistent weight-streaming engine (decode_engine.hip), one launch per layer between the attention launches
    uint32_t* eng_gran = nullptr;                // granule arrays of all layers (zeroed at the head of every forward)
    size_t eng_gran_bytes = 0;
    long eng_forwards = 0;
    // tensor-parallel prefill in two row halves whose all-reduces run on the context's second stream (emu_llama_set_tp_overlap)
    int tp_overlap_rows = 0;                     // 0: off; else the smallest prompt (rows) that takes the two-half schedule
    long ov_forwards = 0;                        // forwards that took it (tests, tools)
};
constexpr int EMU_ARRIVE_INTS = 65536;

namespace {
struct LlamaWs {
    bf16_t *hB, *xn, *qkv, *attn, *act, *vt;
    uint8_t* x8;            // prefill with fp8 weights: the current GEMM's activation rows as e4m3 bytes ...
    float* xs;              // ... and their per-row scales
    float* dec;
    float* splitk;          // prefill only: K-slices of the GEMMs' tail round
    size_t splitk_floats;
    bf16_t* vt2;            // two-lane tensor-parallel prefill (emu_llama_set_tp_overlap): the second lane's own V^T ...
    float* splitk2;         // ... and K-slice scratch (the lanes' GEMMs run concurrently)
    bf16_t* pvt;            // emu_llama_set_kv_prefix: the current layer's prefix V^T [Hl, D, pad64(prefix_len)], one row for all Bn
    size_t total;
};
// chunk: a chunk step of Bn x T rows (emu_llama_forward_chunk) -- no V^T, the split states of every row and the rows' slots
LlamaWs llama_ws(const emu_llama* m, int Bn, int T, void* base, bool chunk = false) {
    const emu_llama_cfg& c = m->cfg;
    const size_t M = (size_t)Bn * T, HD = (size_t)c.heads_local * c.head_dim;
    char* p = reinterpret_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
    LlamaWs w;
    w.hB = (bf16_t*)take(M * c.hidden * 2);
    w.xn = (bf16_t*)take(M * c.hidden * 2);
    w.qkv = (bf16_t*)take(M * 3 * HD * 2);
    w.attn = (bf16_t*)take(M * HD * 2);
    w.act = (bf16_t*)take(M * (size_t)c.ffn_local * 2);
    const size_t spad = (size_t)((m->s_max + 63) / 64) * 64;
    w.vt = (bf16_t*)take(T > 1 && !chunk ? (size_t)Bn * HD * spad * 2 : 0);
    w.dec = (float*)take((chunk ? decode_chunk_ws_floats(Bn, T, c.heads_local, c.head_dim, m->s_max > 0 ? m->s_max : 1)
                                : decode_fused_ws_floats(Bn, c.heads_local, c.head_dim, m->s_max > 0 ? m->s_max : 1)) * sizeof(float));
    w.splitk_floats = M > 16 ? EMU_SPLITK_SCRATCH_FLOATS : 0;
    w.splitk = (float*)take(w.splitk_floats * sizeof(float));
    const size_t kmax = std::max<size_t>(std::max<size_t>(c.hidden, HD), c.ffn_local);
    w.x8 = (uint8_t*)take(M > 16 ? M * kmax : 0);
    w.xs = (float*)take(M > 16 ? M * sizeof(float) : 0);
    const bool lanes = m->tp_overlap_rows > 0 && Bn == 1 && T >= m->tp_overlap_rows;
    w.vt2 = (bf16_t*)take(lanes ? HD * spad * 2 : 0);
    w.splitk2 = (float*)take(lanes ? w.splitk_floats * sizeof(float) : 0);
    w.pvt = (bf16_t*)take(m->prefix_len > 0 && T > 1 && !chunk ? HD * (size_t)((m->prefix_len + 63) / 64 * 64) * 2 : 0);
    w.total = off;
    return w;
}

// out = epi(fp8(A rows, quantised here) x fp8 weights): the prefill form of the fp8 weight set (emu_linear_fp8_bf16)
int linear_q8(const LlamaWs& w, const bf16_t* A, int lda, const uint8_t* W8, const float* wscale, const bf16_t* res, bf16_t* C,
              int M, int N, int K, int ldres, int ldc, int epi, hipStream_t s) {
    int st = launch_quant_fp8_rows(A, lda, w.x8, K, w.xs, M, K, s);
    if (st) return st;
    GemmArgs g{reinterpret_cast<const bf16_t*>(w.x8), reinterpret_cast<const bf16_t*>(W8), nullptr, res, C, M, N, K, K, K, ldres, ldc,
               epi, ConvGeom{0, 0, 0, 0, 0, 0}, nullptr, 0, 0};
    g.a_scale = w.xs; g.w_scale = wscale;
    g.partial = w.splitk; g.partial_floats = w.splitk_floats;
    return launch_gemm_fp8(g, s);
}
// C = epi(A W^T [+ res]) followed by xn = RMSNorm(C) * gain: one row-wise slice-sum launch where the 256x256 tile K-slices every
// tile of the GEMM (GemmArgs::norm_*; launch_gemm answers -95 otherwise), else the GEMM and the rmsnorm launch apart.  Same bits.
int linear_then_rmsnorm(const LlamaWs& w, const bf16_t* A, const bf16_t* W, const bf16_t* res, bf16_t* C, int M, int N, int K, int epi,
                        const bf16_t* gain, bf16_t* xn, float eps, bool fuse, hipStream_t s) {
    if (fuse && M > 16) {
        GemmArgs g{A, W, nullptr, res, C, M, N, K, K, K, N, N, epi, ConvGeom{0, 0, 0, 0, 0, 0}, nullptr, 0, 0};
        g.partial = w.splitk; g.partial_floats = w.splitk_floats;
        g.norm_w = gain; g.norm_out = xn; g.norm_ld = N; g.norm_eps = eps;
        const int st = launch_gemm(g, s);
        if (st != -95) return st;
    }
    int st = linear(A, W, nullptr, res, nullptr, C, M, N, K, K, K, N, N, 0.f, epi, s, nullptr, w.splitk, w.splitk_floats);
    if (st) return st;
    return launch_rmsnorm(C, gain, xn, M, N, N, N, eps, s);
}

// ---- one emu_llama_forward call.  LlamaPlan: which schedule runs it and what that schedule fuses -- pick_path decides; the one
// later change is layer_kv's demotion of fuse_rope when the GEMM refuses the epilogue (-95).  LlamaCall: the arguments and derived sizes every routine of the call shares, and one routine per schedule.
enum class LlamaPath { Launches, Engine, FusedLayers, FusedCutAtAllReduce, FusedTailAllReduce, TwoLane };
struct LlamaPlan {
    LlamaPath path;
    // fuse_rope      the qkv GEMM's epilogue rotates q / k, appends k / v and writes V^T (demoted for the rest of the call on -95)
    // fuse_norm      the K-slice sums of o_proj / down_proj apply the RMSNorm behind them
    // kernel         the weight set and kernel of the call's projections (call_kernel).  Fp8Gemm: in the layers that have fp8
    //                weights.  Fp4Thin, Fp8Thin: norms stay launches.  A kernel without a bf16 GEMM behind it (KERNEL_FACTS: Fp4Gemm,
    //                Fp8Stream, Fp8Tile): norms, RoPE / KV append and V^T stay launches -- fuse_rope and fuse_norm are off, never TwoLane
    // norm_in_gemv   one row, or two with fp8 / fp4 weights: the weight stream applies the RMSNorm in front of it itself
    // decode_tail    decode attention without the combine launch (emu_llama_set_decode_tail)
    // merge_o        the o_proj launch merges the decode attention's splits (emu_gemm_tune bit 19)
    WeightKernel kernel;
    bool fuse_rope, fuse_norm, norm_in_gemv, decode_tail, merge_o;
    // warm           boundaries of the layer whose predecessor warms the XCDs' L2s with the head of its successor (emu_llama_set_l2_warm's
    //                bits 0-4); only the default one-row step has any: bf16 weights, no tensor parallelism, own KV rows, the combine launch
    int warm = 0;
    // the launch arguments as far as they are decided here -- Fused*: H, Hl, Fl, the wait bound and the peers' comm blocks (tp_n == 0:
    // no all-reduce inside a launch); Engine: the engine areas of the comm blocks (comm, seq, tp_n, tp_rank)
    DecodeLayersArgs dl; EngArgs eng;
};
// a window of the call's rows that one stream walks through a layer: every row on the caller's stream (run_launches), or one
// lane's half of a long prompt (llama_prefill_lanes)
struct RowWindow {
    int r0, T, kend;                             // first row; rows per batch element; the window's last row sees keys [0, kend)
    hipStream_t s;
    LlamaWs w;                                   // the call's buffers at row r0; V^T and the K-slice scratch are the window's own
    bf16_t* x; const int32_t *pos, *slot;        // the residual stream and the rows' positions / cache slots, at row r0
    std::function<int(bf16_t*, size_t)> allreduce;   // sums partial rows over the ranks, in the window's stream
};
using LaneHook = std::function<int()>;           // what a schedule issues between two launches of the layer body (events of the two lanes)
struct LlamaCall {
    emu_llama* m; emu_ctx* cx; LlamaWs ws; hipStream_t s;
    bf16_t* hA;                                  // the residual stream, [M, H]
    const int32_t *pos, *slot, *kstart;
    int Bn, T, M, ctx, H, Hl, D, HD, Fl, spad, l_end;
    bool tp;                                     // a 1-rank communicator / comm block still runs the all-reduces (tests, tools/tp_emulate.py)
    int epi_res;                                 // the residual enters the all-reduce once: rank 0 adds it
    float scale, eps; size_t kv_layer;
    LlamaPlan plan;
    bool xn_ready;                               // the down projection of the layer before left this layer's normalised rows in w.xn
    bool chunk = false;                          // emu_llama_forward_chunk: pos / slot are pos0 / slot0 [Bn], row i of a sequence sits i behind them

    // The chunk step's plan: the per-layer launches, the projections by whatever kernel_for(Bn * T) plans, no fusion that belongs to
    // the prompt or to the one-row step.
    void plan_chunk() {
        LlamaPlan& p = plan = LlamaPlan{};
        p.path = LlamaPath::Launches;
        p.kernel = m->kernel_for(M);
        p.fuse_rope = p.fuse_norm = p.decode_tail = p.merge_o = false;
        p.norm_in_gemv = norm_rides(p.kernel);
    }

    // Decides the call's schedule and fusions; launches, zeroes and uploads nothing.  Precedence: the engine, whole layers per launch,
    // the two-lane prefill, the per-layer launches -- a schedule whose guard fails falls through to the next.
    void pick_path(bool promise) {
        LlamaPlan& p = plan = LlamaPlan{};
        p.path = LlamaPath::Launches;                  // unless a schedule below takes the call
        const bool own_kv = m->kv_share_nb <= 1, some_layers = l_end > m->l0;
        // the caller promised (emu_llama_set_prefill_fusion) that the rows of the one batch element are the whole context in slot
        // order, slot[i] = i.  The promise is per call: emu_llama_forward consumed it, so a later forward with rows in another slot
        // order (any caller that did not renew it) runs the unfused sequence, which honours slot[] everywhere.
        // (a KV prefix: the rows are a continuation behind the prefix, whatever T == ctx and slots 0 .. T - 1 look like -- never fused)
        const bool ordered_prompt = promise && Bn == 1 && T == ctx && !fp8_prefill(m->mode) && own_kv && m->prefix_len == 0;
        // Prefill of such a prompt: the qkv projection rotates q / k, appends k / v to the cache and writes V^T itself
        // (GemmArgs::rope_*), instead of the rope_kv and transpose_v launches.
        p.kernel = m->kernel_for(M);
        // else: no bf16 GEMM to carry an epilogue fusion or the two lanes (which start at 512 rows, where only Fp4Gemm lacks one)
        const bool bf16_gemm = facts(p.kernel).bf16_gemm;
        p.fuse_rope = ordered_prompt && T > 16 && D == 128 && !(HD & 255) && bf16_gemm;
        // (prefill fusion, no tensor parallelism: the K-slice sums of o_proj / down_proj apply the RMSNorm that follows them; for
        // down_proj that is the NEXT layer's input norm, so a layer may find its normalised rows in w.xn already)
        // The K-slice sum + RMSNorm fusion does not depend on the slot order: it follows the sticky capability (fuse_norm_on: set with the
        // first promise, cleared by emu_llama_set_prefill_fusion(0)), so M > 16 rows of single-token steps (beam / contrastive search
        // with B * beams > 16) keep the fused path they had before the promise became one-shot.
        p.fuse_norm = m->fuse_norm_on && !tp && M > 16 && !fp8_prefill(m->mode) && bf16_gemm;
        p.norm_in_gemv = norm_rides(p.kernel) || M == 1;
        p.decode_tail = T == 1 && m->decode_tail && m->arrive && own_kv && (long)Bn * Hl <= EMU_ARRIVE_INTS;
        // short shards (a TP = 8 rank's 7 heads), opt-in (emu_gemm_tune bit 19): the o_proj launch merges the attention's splits
        // itself, no combine launch (gemv_merge.hip).  Bit-identical and measured LEVEL with the two launches (3.15 vs 3.15-3.18 ms
        // per token of a TP = 8 shard, profiles/r05_tp_emulate_merged_o_proj.log): the merge is a dependent L2 trip inside the
        // projection, which is what the combine launch cost -- one launch less buys nothing here, like the in-kernel split merge
        // and the tail all-reduce before it
        p.merge_o = T == 1 && M == 1 && p.kernel == WeightKernel::Bf16 && !p.decode_tail && own_kv && gemv_merge_ok(Hl, D, H, (ctx + 127) / 128) &&
                    (emu_gemm_tune_get() & (1 << 19)) != 0;
        if (T == 1 && M == 1 && p.kernel == WeightKernel::Bf16 && !tp && own_kv && !p.decode_tail && !p.merge_o && !m->decode_fused &&
            !(emu_gemm_tune_get() & (1 << 30)))
            p.warm = m->l2_warm;

        const bool one_row_bf16 = T == 1 && Bn == 1 && D == 128 && !quantised(m->mode) && own_kv && some_layers;
        // the fence-free peer-to-peer all-reduce is on (which implies tensor parallelism and an opened cx->p2p): what the all-reduces
        // inside a launch build on
        const bool p2p_fence_free = cx->p2p_on && emu_p2p_fenced(cx->p2p) == 0;
        // ---- the persistent weight-streaming engine (mode 4; run_engine).  Tensor-parallel shards with rows of at most 13 KiB (TP >= 4)
        // whose ranks have the device to themselves; anything else takes the launches.
        if (m->decode_fused == 4 && one_row_bf16 && m->eng_gran && m->dl_err && p2p_fence_free && H <= 6656 && HD <= 6656 && Fl <= 6656 &&
            !(H & 7) && !(Fl & 7) && emu_p2p_engine_view(cx->p2p, p.eng.comm, &p.eng.seq, &p.eng.tp_n, &p.eng.tp_rank) && cx->ncu > 0 &&
            3 * HD >= 2 * cx->ncu && H >= 2 * cx->ncu && Fl >= cx->ncu && cx->ncu <= 1024) { p.path = LlamaPath::Engine; return; }
        // ---- whole layers per launch (modes 1 to 3; run_fused_layers)
        if (m->decode_fused && m->decode_fused != 4 && one_row_bf16 && m->dl_cnt) {
            DecodeLayersArgs& d = p.dl;
            d.H = H; d.Hl = Hl; d.Fl = Fl;
            bool ok = decode_layers_ok(d);
            // wait bound: 2 s of wall clock (100 MHz ticks), or the peer-to-peer time-out where that is longer -- rank processes that SHARE
            // a GPU (validation runs) are time-sliced against each other, and a wave that is switched out keeps its start time: the 0.2 s
            // of the first version ran out under eight ranks on one device (garbage from step 4 on, give-ups counted)
            d.limit_ticks = 200000000LL;
            // tensor parallelism: mode 2 runs the all-reduces inside the launch over the P2P comm blocks (every rank on its own GPU); mode 1
            // cuts every layer at its two all-reduces -- [q, attention, o_proj] | all-reduce | [gate/up, down] | all-reduce -- which also
            // serves RCCL and ranks that share a GPU (a launch that waits for a peer must not hold the CUs the peer needs); mode 3 leaves
            // each all-reduce to the last workgroup of the projection's launch, and falls back to the cut where that is not available
            bool in_kernel_ar = false, tail_ar = false;
            if (ok && tp && cx->p2p) {
                long long lim = 0; int n = 0;
                const bool view = emu_p2p_view(cx->p2p, d.tp_block, &d.tp_seq, &n, &d.tp_rank, &lim);
                in_kernel_ar = view && p2p_fence_free && m->decode_fused == 2;       // the in-launch all-reduce is the fence-free form only
                tail_ar = view && p2p_fence_free && m->decode_fused == 3;
                if (view && lim > d.limit_ticks) d.limit_ticks = lim;  // a lagging peer holds every downstream wait: the peer bound applies
                d.tp_n = in_kernel_ar ? n : 0;
                ok = decode_layers_ok(d);
                if (tail_ar) d.tp_n = n;                               // (launch_decode_layers checks the shape for the launches that all-reduce)
            }
            if (ok) p.path = tail_ar ? LlamaPath::FusedTailAllReduce : tp && !in_kernel_ar ? LlamaPath::FusedCutAtAllReduce : LlamaPath::FusedLayers;
            if (ok) return;
        }
        // ---- long prompt under tensor parallelism: two row halves, every all-reduce behind the other half's GEMMs (needs the slot-order
        // promise: the rows of the one batch element are the whole context in order, so the first half never reads the second's keys)
        if (bf16_gemm && tp && m->tp_overlap_rows > 0 && cx->lane_stream && cx->ar_ev[4] && ws.vt2 && ordered_prompt && M >= m->tp_overlap_rows && some_layers)
            p.path = LlamaPath::TwoLane;
    }

    // One projection of a layer, C = epi(A W^T [+ res]): qkv, o_proj, gate/up and down all come through here, from the matrix's record
    // by the plan's kernel (every window of a call has the row range the plan chose it for: pick_path).  gain_in: the RMSNorm in front,
    // fused into a one-row weight stream; gain_out: w.xn = RMSNorm(C) * gain_out behind the K-slice sums.
    int project(const LlamaWs& w, hipStream_t s, const bf16_t* A, const Weights& W, const bf16_t* res, const bf16_t* gain_in,
                const bf16_t* gain_out, bf16_t* C, int rows, int N, int K, int epi, const WarmPlan& warm = WarmPlan{}) {
        const int ldres = res ? N : 0, ldc = epi == EPI_SWIGLU ? N / 2 : N;
        if (facts(plan.kernel).bf16_gemm && !W.W && !(plan.kernel == WeightKernel::Fp8Gemm && W.W8 && m->mode.bf16_released)) return fail(cx, -22, "emu_llama_forward: bf16 layer weights not set (released by emu_llama_release_bf16?)");
        emu_projection q = m->site(W, rows, N, K, gain_in != nullptr, epi, plan.decode_tail, plan.warm | (int)warm.ntouch);   // (the call's plan)
        const WeightKernel k = matrix_kernel(plan.kernel, q);
        if (k == WeightKernel::Fp8Gemm) return linear_q8(w, A, K, W.W8, W.s8, res, C, rows, N, K, ldres, ldc, epi, s);
        if (k == WeightKernel::Bf16 && gain_out) return linear_then_rmsnorm(w, A, W.W, res, C, rows, N, K, epi, gain_out, w.xn, eps, true, s);
        GemvArgs g = packed(k, A, K, gain_in, eps, res, ldres, C, ldc, rows, N, K, epi);
        if (warm.ntouch && k == WeightKernel::Bf16) { g.warm = warm; ++m->warm_launches; }
        return linear_w(k, W, g, s, w.splitk, w.splitk_floats, m->mode.pack_wide);
    }

    // ---- L2 warming (l2_warm.h).  The budget and the head's shape ride in the mask (include/emu_hip.h: emu_llama_set_l2_warm).
    uint64_t warm_budget() const { const int mib = (plan.warm >> 8) & 0xff; return (uint64_t)(mib ? mib : EMU_L2_WARM_DEFAULT_MIB) << 20; }
    int warm_shape() const { return plan.warm & 32 ? WARM_FIRST_TRIP : WARM_WHOLE_BLOCKS; }
    // the packed [N, K] matrix Wn as the one-row stream that follows reads it (emu_gemv_geometry: the rule launch_gemv applies)
    static WarmSucc warm_succ(const bf16_t* Wn, int N, int K, bool norm, int epi) {
        WarmSucc su;
        su.base = Wn; su.rows = (uint32_t)emu_gemv_geometry(N, K, norm, epi).rows; su.row_bytes = su.used_bytes = (uint32_t)K * 2;
        su.nrows = (uint64_t)N;
        return su;
    }
    // boundary `bit`: the one-row stream over [N, K] (a form that carries the loop, else no plan) warms su from its last workgroups
    WarmPlan warm_from_gemv(int bit, int N, int K, bool norm, int epi, const WarmSucc& su) const {
        if (!(plan.warm & (1 << bit)) || !su.base) return WarmPlan{};
        const GemvGeom g = emu_gemv_geometry(N, K, norm, epi);
        if (!gemv_form_warms(g.form)) return WarmPlan{};
        return make_warm_plan(su, (uint32_t)((N + g.rows - 1) / g.rows), false, 256, warm_budget(), warm_shape());
    }

    RowWindow window(int r0, int T, int kend, hipStream_t s, bf16_t* vt, float* splitk) {
        LlamaWs w = ws;
        w.hB += (size_t)r0 * H; w.xn += (size_t)r0 * H; w.qkv += (size_t)r0 * 3 * HD; w.attn += (size_t)r0 * HD; w.act += (size_t)r0 * Fl;
        w.vt = vt; w.splitk = splitk;
        return RowWindow{r0, T, kend, s, w, hA + (size_t)r0 * H, pos + r0, slot + r0, nullptr};
    }
    // ---- The decoder layer, written once, in three steps that are cut where the schedules hook in:
    //     layer_kv      RMSNorm, [after_norm], qkv projection (+ RoPE / KV append / V^T in its epilogue, else the rope_kv launch): the
    //                   window's K / V are cached
    //     layer_attend  [V^T], [after_vt], attention, o_proj, all-reduce
    //     layer_mlp     RMSNorm, gate/up + SwiGLU, down, all-reduce
    int layer_kv(const RowWindow& win, int l, const LaneHook& after_norm = nullptr) {
        const LlamaWs& w = win.w;
        const emu_llama::Layer& L = m->layers[l];
        if (needs_fp8(plan.kernel) && !L.qkv.W8)
            return fail(cx, -22, "emu_llama_forward: fp8 decode enabled but fp8 layer weights not set");
        // after emu_llama_release_bf16 the 4-bit set (mode 3 pinned) or the fp8 set (modes 5 / 6 with fp8_all pinned) is the layer's
        // weights: every row count has a path on it
        if (m->mode.bf16_released ? !(m->mode.fp8_all ? L.qkv.W8 : L.qkv.W4) || !L.ln1 : !L.qkv.W) return fail(cx, -22, "emu_llama_forward: layer weights not set");
        const int rows = Bn * win.T;
        bf16_t *kc = m->kcache + l * kv_layer, *vc = m->vcache + l * kv_layer;
        if (!plan.norm_in_gemv) {                        // 2..16 rows: norm once, skinny MFMA stream; more: GEMM
            if (!xn_ready) TRY(cx, launch_rmsnorm(win.x, L.ln1, w.xn, rows, H, H, H, eps, win.s));
            xn_ready = false;
        }
        if (after_norm) TRY(cx, after_norm());
        int st = -95;
        if (plan.fuse_rope) {
            GemmArgs g{w.xn, L.qkv.W, nullptr, nullptr, w.qkv, rows, 3 * HD, H, H, H, 0, 3 * HD, EPI_NONE, ConvGeom{0, 0, 0, 0, 0, 0}, nullptr, 0, 0};
            g.partial = w.splitk; g.partial_floats = w.splitk_floats;
            g.rope_cos = m->cos; g.rope_sin = m->sin; g.rope_pos = win.pos; g.rope_slot = win.slot; g.rope_kc = kc; g.rope_vc = vc;
            g.rope_hl = Hl; g.rope_smax = m->s_max;
            g.vt_out = w.vt + win.r0; g.vt_col0 = 2 * HD; g.vt_s = rows; g.vt_spad = spad;   // key index = row index: column r0 + m
            st = launch_gemm(g, win.s);
            if (st != 0 && st != -95) return fail(cx, st, "emu_llama_forward: qkv projection with the RoPE epilogue");
            if (st == -95) plan.fuse_rope = false;       // the 256x256 tile does not take this shape unsliced: unfused sequence from here on
        }
        if (st == -95) {
            WarmPlan wp;
            if (plan.warm & 16) {                        // this layer's cache rows as the attention grid (split, head) reads them
                WarmSucc su;
                su.base = kc; su.twin = (int64_t)(vc - kc) * 2; su.rows = 128; su.row_bytes = su.used_bytes = (uint32_t)D * 2;
                su.nrows = (uint64_t)m->s_max; su.gx = (uint32_t)((ctx + 127) / 128); su.groups = (uint32_t)Hl;
                if (D == 128) wp = warm_from_gemv(4, 3 * HD, H, true, EPI_NONE, su);
            }
            TRY(cx, project(w, win.s, plan.norm_in_gemv ? win.x : w.xn, L.qkv, nullptr, plan.norm_in_gemv ? L.ln1 : nullptr,
                            nullptr, w.qkv, rows, 3 * HD, H, EPI_NONE, wp));
        }
        if (T == 1 || chunk) return 0;                   // single-token and chunk steps: the attention launch rotates and appends
        if (m->kv_share_nb > 1) return fail(cx, -22, "emu_llama_forward: shared-prefix KV rows serve single-token steps only");
        if (plan.fuse_rope) return 0;
        RopeKvArgs r{w.qkv, m->cos, m->sin, win.pos, win.slot, kc, vc, Bn, win.T, Hl, D, m->s_max};
        TRY(cx, launch_rope_kv(r, win.s));
        return 0;
    }

    int layer_attend(const RowWindow& win, int l, const LaneHook& after_vt = nullptr) {
        const LlamaWs& w = win.w;
        const emu_llama::Layer& L = m->layers[l];
        const int rows = Bn * win.T;
        bf16_t *kc = m->kcache + l * kv_layer, *vc = m->vcache + l * kv_layer;
        if (chunk) {
            // the same for T rows per sequence at consecutive slots (attention.hip: decode_chunk_kernel)
            DecodeChunkArgs a{w.qkv, m->cos, m->sin, win.pos, win.slot, kc, vc, w.attn, (long)HD, (long)D, kstart, w.dec,
                              Bn, win.T, Hl, D, m->s_max, ctx, scale};
            TRY(cx, launch_decode_chunk(a, win.s));
        } else if (T == 1) {
            // RoPE + KV append + attention in one launch; context = slot + 1 is read on the device (graph replay)
            DecodeFusedArgs a{w.qkv, m->cos, m->sin, win.pos, win.slot, kc, vc, w.attn, (long)HD, (long)D, kstart, w.dec,
                              Bn, Hl, D, m->s_max, ctx, scale, m->kv_share_nb, m->kv_share_len};
            if (plan.decode_tail) a.arrive = m->arrive;
            a.skip_combine = plan.merge_o;
            if ((plan.warm & 1) && Bn == 1 && L.o.W) {   // extra workgroups of the combine launch warm o_proj
                a.warm = make_warm_plan(warm_succ(L.o.W, H, HD, false, epi_res), (uint32_t)Hl, true, (uint32_t)D, warm_budget(), warm_shape());
                if (a.warm.ntouch) ++m->warm_launches;
            }
            TRY(cx, launch_decode_fused(a, win.s));
        } else {
            if (!plan.fuse_rope) {
                TransposeVArgs tv{vc, (long)Hl * m->s_max * D, (long)m->s_max * D, (long)D, w.vt, Bn, Hl, win.kend, D, spad};
                TRY(cx, launch_transpose_v(tv, win.s));      // keys [0, kend) key-contiguous, zero up to spad
            }
            if (after_vt) TRY(cx, after_vt());
            if (m->prefix_len > 0) {
                // two segments: the prefix's keys from its own cache (V^T of ONE row, once per layer), then the rows' own slots [0, kend)
                const int P = m->prefix_len, ppad = (P + 63) / 64 * 64;
                const size_t pl = (size_t)Hl * m->prefix_s_max * D;
                TransposeVArgs tp_{m->vprefix + l * pl, (long)pl, (long)m->prefix_s_max * D, (long)D, w.pvt, 1, Hl, P, D, ppad};
                TRY(cx, launch_transpose_v(tp_, win.s));
                FlashPrefixArgs pa{w.qkv, (long)win.T * 3 * HD, (long)D, (long)3 * HD,
                                   m->kprefix + l * pl, (long)m->prefix_s_max * D, (long)D, w.pvt,
                                   kc, (long)Hl * m->s_max * D, (long)m->s_max * D, (long)D, w.vt,
                                   w.attn, (long)win.T * HD, (long)D, (long)HD, kstart, 0,
                                   Bn, Hl, win.T, P, ppad, win.kend, spad, D, scale};
                TRY(cx, launch_flash_attn_prefix(pa, win.s));
            } else {
                FlashArgs fa{w.qkv, (long)win.T * 3 * HD, (long)D, (long)3 * HD,
                             kc, (long)Hl * m->s_max * D, (long)m->s_max * D, (long)D,
                             w.vt, w.attn, (long)win.T * HD, (long)D, (long)HD, kstart,
                             Bn, Hl, win.T, win.kend, spad, D, 1, scale};          // query i of the window sees keys <= r0 + i
                TRY(cx, launch_flash_attn(fa, win.s));
            }
        }
        if (plan.merge_o) {
            GemvMergeArgs g{w.dec, win.slot, (ctx + 127) / 128, Hl, L.o.W, win.x, w.hB, H, HD, HD, epi_res, nullptr};
            TRY(cx, gemv_merge_profiled(g, win.s));
        } else
            TRY(cx, project(w, win.s, w.attn, L.o, win.x, nullptr, plan.fuse_norm ? L.ln2 : nullptr, w.hB, rows, H, HD, epi_res,
                            warm_from_gemv(1, H, HD, false, epi_res, warm_succ(L.gu.W, 2 * Fl, H, true, EPI_SWIGLU))));
        return win.allreduce(w.hB, (size_t)rows * H);
    }

    int layer_mlp(const RowWindow& win, int l) {
        const LlamaWs& w = win.w;
        const emu_llama::Layer& L = m->layers[l];
        const int rows = Bn * win.T;
        if (!plan.norm_in_gemv && !plan.fuse_norm) TRY(cx, launch_rmsnorm(w.hB, L.ln2, w.xn, rows, H, H, H, eps, win.s));
        TRY(cx, project(w, win.s, plan.norm_in_gemv ? w.hB : w.xn, L.gu, nullptr, plan.norm_in_gemv ? L.ln2 : nullptr, nullptr,
                        w.act, rows, 2 * Fl, H, EPI_SWIGLU,
                        warm_from_gemv(2, 2 * Fl, H, true, EPI_SWIGLU, warm_succ(L.down.W, H, Fl, false, epi_res))));
        // (fuse_norm: the RMSNorm behind down_proj is the NEXT layer's input norm, which then finds its rows in w.xn)
        const bf16_t* next_ln1 = plan.fuse_norm && l + 1 < l_end ? m->layers[l + 1].ln1 : nullptr;
        // (behind the model's last layer the whole head follows: emu_llama_logits' one-row stream with the final norm in front)
        WarmSucc after;
        if (l + 1 < l_end) after = warm_succ(m->layers[l + 1].qkv.W, 3 * HD, H, true, EPI_NONE);
        else if (l + 1 == m->cfg.layers && m->head_rows < 0 && m->final_norm) after = warm_succ(m->head.W, m->cfg.vocab, H, true, EPI_NONE);
        TRY(cx, project(w, win.s, w.act, L.down, w.hB, nullptr, next_ln1, win.x, rows, H, Fl, epi_res,
                        warm_from_gemv(3, H, Fl, false, epi_res, after)));
        if (next_ln1) xn_ready = true;
        return win.allreduce(win.x, (size_t)rows * H);
    }

    // ---- the per-layer launches: every row of the call on the caller's stream
    int run_launches() {
        RowWindow win = window(0, T, ctx, s, ws.vt, ws.splitk);
        win.allreduce = [this](bf16_t* buf, size_t n) { return tp ? emu_allreduce_bf16(cx, buf, n, reinterpret_cast<emu_stream_t>(s)) : 0; };
        for (int l = m->l0; l < l_end; ++l) {
            TRY(cx, layer_kv(win, l));
            TRY(cx, layer_attend(win, l));
            TRY(cx, layer_mlp(win, l));
        }
        return 0;
    }

    // ---- Tensor-parallel prefill of a long prompt as TWO CONCURRENT LANES (SURVEY 8e / north_star: "all-reduce overlapped with the
    // next GEMM"; replaces the serial schedule of run_launches).  The prompt's rows are cut once, at a multiple of 256
    // (whole 256-row GEMM tiles and whole 64-key attention tiles below the cut), into A = [0, Ma) and B = [Ma, M).  Causal attention
    // makes A independent of B, and B needs nothing of A but its keys / values of the SAME layer, so each half walks all layers as its
    // own chain
    //     [RMSNorm, qkv (+ RoPE / KV append / V^T), attention, o_proj] -> all-reduce -> [RMSNorm, gate/up + SwiGLU, down] -> all-reduce
    // on its own stream: A on the caller's, B on cx->lane_stream, one event per layer (A's K / V rows are in the cache) the only edge
    // between them.  While one lane's partial sums are on the wire the other lane's GEMMs have the CUs, and where both lanes compute,
    // their launches (a TP = 8 shard's GEMM over 772 rows is 30-odd tiles on 256 CUs) share the chip instead of queueing behind each
    // other.  A first version kept ONE compute stream and interleaved the halves stage by stage with every all-reduce on a side
    // stream: +43 % per rank on one GPU (profiles/r05_tp_prefill_two_half_v1_single_compute_stream.log) -- half-size launches back to
    // back leave most of the chip idle, and every all-reduce cost two cross-stream edges.  All-reduces run in their lane's stream
    // where RCCL takes them (one communicator, calls in one host order on every rank); on a context without a communicator (rank
    // processes sharing a device: validation) every peer-to-peer all-reduce additionally waits for the one issued before it in
    // either lane, because the comm blocks serve one all-reduce at a time.  Lane B keeps its own V^T buffer (A's keys transposed from the cache + its own columns
    // from the epilogue) and K-slice scratch, so no buffer is written by one lane while the other reads it.  Same kernels and
    // rounding points as the serial schedule; a half may take another GEMM tile configuration than the whole prompt (K-slice sums in
    // another order), so the schedules agree to bf16 rounding, not bit for bit.  Capturable: lane_stream forks from and joins the
    // caller's stream through events.
    int llama_prefill_lanes() {
        const int Ma = (M / 2 + 128) / 256 * 256;        // M >= 512 (emu_llama_set_tp_overlap, pick_path): 256 <= Ma <= M - 256
        hipStream_t lane[2] = {s, cx->lane_stream};
        RowWindow win[2] = {window(0, Ma, Ma, lane[0], ws.vt, ws.splitk), window(Ma, M - Ma, M, lane[1], ws.vt2, ws.splitk2)};
        hipEvent_t eStart = cx->ar_ev[0], eKV = cx->ar_ev[1];              // (ar_ev[2]: the join in llama_prefill_overlapped)
        hipEvent_t* ePrev = cx->ar_ev + 3;   // [lane]  the lane's latest peer-to-peer all-reduce is through (an event is only ever recorded on
        int prev_lane = -1;                  //         ONE stream: one event recorded on both streams of a capture crashed hipGraphInstantiate)
#define HIPTRY(expr) do { if ((expr) != hipSuccess) { (void)hipGetLastError(); return fail(cx, -5, #expr); } } while (0)
        auto lane_allreduce = [&](int h, bf16_t* buf, size_t n) -> int {
            const bool by_rccl = cx->comm && !(cx->p2p_on && n * sizeof(bf16_t) <= EMU_P2P_SLOT_BYTES);   // emu_allreduce_bf16's own choice
            if (by_rccl) return emu_allreduce_bf16(cx, buf, n, reinterpret_cast<emu_stream_t>(lane[h]));
            // the comm blocks serve ONE all-reduce at a time: every peer-to-peer all-reduce waits for the one issued before it (host order,
            // the same on every rank), whichever lane that was in
            if (prev_lane >= 0 && prev_lane != h) HIPTRY(hipStreamWaitEvent(lane[h], ePrev[prev_lane], 0));
            TRY(cx, emu_allreduce_bf16(cx, buf, n, reinterpret_cast<emu_stream_t>(lane[h])));
            HIPTRY(hipEventRecord(ePrev[h], lane[h]));
            prev_lane = h;
            return 0;
        };
        for (int h = 0; h < 2; ++h) win[h].allreduce = [&lane_allreduce, h](bf16_t* buf, size_t n) { return lane_allreduce(h, buf, n); };
        HIPTRY(hipEventRecord(eStart, lane[0]));                             // inputs (and whatever the caller queued before) are ready
        HIPTRY(hipStreamWaitEvent(lane[1], eStart, 0));
        for (int l = m->l0; l < l_end; ++l) {
            // Host order per layer: A.attention, B.attention, A.mlp, B.mlp -- so B's wait for eKV sees A's record of this layer, and the
            // all-reduces are issued in the order o_A, o_B, down_A, down_B.  The order matters beyond bookkeeping: all-reduces of one
            // communicator run in issue order (RCCL makes a call on another stream wait for the stream of the call before it; the
            // peer-to-peer chain above does the same), so an all-reduce can only wait for work issued ahead of it.  Issued lane by lane
            // (A's whole layer, then B's), B's first all-reduce would wait for A's second and the lanes would take turns instead of overlapping.
            // lane B's V^T with the RoPE epilogue: A's keys of this layer out of the cache (zero behind them), between B's RMSNorm and
            // its qkv GEMM, whose epilogue adds B's own columns
            const LaneHook keys_of_A = [&]() -> int {
                HIPTRY(hipStreamWaitEvent(lane[1], eKV, 0));
                TransposeVArgs tv{m->vcache + l * kv_layer, (long)Hl * m->s_max * D, (long)m->s_max * D, (long)D, ws.vt2, 1, Hl, Ma, D, spad};
                return launch_transpose_v(tv, lane[1]);
            };
            // K / V rows [0, Ma) of layer l are in the cache: recorded behind A's qkv GEMM, or behind A's transpose_v in the unfused sequence
            const LaneHook kv_of_A_cached = [&]() -> int { HIPTRY(hipEventRecord(eKV, lane[0])); return 0; };
            for (int h = 0; h < 2; ++h) {
                // (-95 from the fused qkv GEMM: the unfused sequence from there on, in both lanes)
                TRY(cx, layer_kv(win[h], l, h == 1 && plan.fuse_rope ? keys_of_A : LaneHook()));
                if (h == 1 && !plan.fuse_rope) HIPTRY(hipStreamWaitEvent(lane[1], eKV, 0));   // layer_attend transposes keys [0, M) out of the cache
                TRY(cx, layer_attend(win[h], l, h == 0 ? kv_of_A_cached : LaneHook()));
            }
            for (int h = 0; h < 2; ++h) TRY(cx, layer_mlp(win[h], l));
        }
#undef HIPTRY
        return 0;
    }
    int llama_prefill_overlapped() {
        const int st = llama_prefill_lanes();
        // join, on the error path as well: whatever reached the second lane is ordered ahead of the caller's next launch (and a stream
        // capture in progress ends with the lane joined); the caller's stream owns the residual stream again
        const bool joined = hipEventRecord(cx->ar_ev[2], cx->lane_stream) == hipSuccess && hipStreamWaitEvent(s, cx->ar_ev[2], 0) == hipSuccess;
        if (st != 0) return st;
        if (!joined) { (void)hipGetLastError(); return fail(cx, -5, "emu_llama_forward: joining the second lane"); }
        ++m->ov_forwards;
        return 0;
    }

    // ---- one-row step with bf16 weights on the persistent weight-streaming engine (decode_engine.hip; mode 4): per layer the attention
    // launches, then ONE launch for  o_proj -> all-reduce -> RMSNorm + gate/up (SwiGLU) -> down -> all-reduce -> RMSNorm + the NEXT
    // layer's qkv projection, the weight stream running ahead of the four hand-offs; same bits as the launches of run_launches.
    int run_engine() {
        const LlamaWs& w = ws;
        EngArgs e = plan.eng;
        e.err = m->dl_err; e.ncu = cx->ncu;
        engine_tool_switches(e);
        for (int l = m->l0; l < l_end; ++l)
            if (!m->layers[l].qkv.W) return fail(cx, -22, "emu_llama_forward: layer weights not set");
        if (hipMemsetAsync(m->eng_gran, 0, m->eng_gran_bytes, s) != hipSuccess) return fail(cx, -5, "emu_llama_forward: hipMemsetAsync");
        const size_t gH = align_up((size_t)H * 4), gF = align_up((size_t)Fl * 4);
        const bool res_here = epi_res == EPI_RESID;           // rank 0 adds the residuals (they enter the all-reduce once)
        // the first layer's qkv projection is a launch of its own
        TRY(cx, project(w, s, hA, m->layers[m->l0].qkv, nullptr, m->layers[m->l0].ln1, nullptr, w.qkv, 1, 3 * HD, H, EPI_NONE));
        for (int l = m->l0; l < l_end; ++l) {
            const emu_llama::Layer& L = m->layers[l];
            bf16_t *kc = m->kcache + l * kv_layer, *vc = m->vcache + l * kv_layer;
            DecodeFusedArgs da{w.qkv, m->cos, m->sin, pos, slot, kc, vc, w.attn, (long)HD, (long)D, kstart, w.dec, Bn, Hl, D, m->s_max, ctx, scale, 0, 0};
            TRY(cx, launch_decode_fused(da, s));
            const bool last = l + 1 == l_end;
            char* gl = reinterpret_cast<char*>(m->eng_gran) + (size_t)l * (2 * gH + gF);
            uint32_t* g_hb = reinterpret_cast<uint32_t*>(gl);
            uint32_t* g_act = reinterpret_cast<uint32_t*>(gl + gH);
            uint32_t* g_ha = reinterpret_cast<uint32_t*>(gl + gH + gF);
            int k = 0;
            EngOp& o0 = e.op[k++] = EngOp{};                          // o_proj: partial sums of the post-attention stream
            o0.W = L.o.W; o0.N = H; o0.K = HD; o0.epi = res_here ? EPI_RESID : EPI_NONE; o0.res = hA; o0.res_src = 0;
            o0.vw = emu_gemv_partition(H, HD, false, epi_res); o0.x_src = 0; o0.xg = w.attn; o0.out_dst = 2; o0.ar_k = 0;
            EngOp& o1 = e.op[k++] = EngOp{};                          // all-reduce -> RMSNorm -> gate / up -> SwiGLU
            o1.W = L.gu.W; o1.N = 2 * Fl; o1.K = H; o1.gain = L.ln2; o1.eps = eps; o1.epi = EPI_SWIGLU;
            o1.vw = emu_gemv_partition(2 * Fl, H, true, EPI_SWIGLU); o1.x_src = 2; o1.xgran = g_hb; o1.ar_k = 0; o1.keep_raw = 1;
            o1.out_dst = 1; o1.ogran = g_act;
            EngOp& o2 = e.op[k++] = EngOp{};                          // down: partial sums of the layer output (+ the summed stream on rank 0)
            o2.W = L.down.W; o2.N = H; o2.K = Fl; o2.epi = res_here ? EPI_RESID : EPI_NONE; o2.res_src = 1;
            o2.vw = emu_gemv_partition(H, Fl, false, epi_res); o2.x_src = 1; o2.xgran = g_act;
            if (!last) {
                o2.out_dst = 2; o2.ar_k = 1;
                EngOp& o3 = e.op[k++] = EngOp{};                      // all-reduce -> RMSNorm -> the NEXT layer's qkv projection
                const emu_llama::Layer& Ln = m->layers[l + 1];
                o3.W = Ln.qkv.W; o3.N = 3 * HD; o3.K = H; o3.gain = Ln.ln1; o3.eps = eps; o3.epi = EPI_NONE;
                o3.vw = emu_gemv_partition(3 * HD, H, true, EPI_NONE); o3.x_src = 2; o3.xgran = g_ha; o3.ar_k = 1; o3.sum_out = hA;
                o3.out_dst = 0; o3.out = w.qkv;
                e.n_ar = 2;
            } else {
                o2.out_dst = 0; o2.out = hA;                // the last layer's output leaves as this rank's partial sums
                e.n_ar = 1;
            }
            e.nops = k;
            const int st = launch_decode_engine(e, s);
            if (st) return fail(cx, st, "emu_llama_forward: decode engine launch");
            if (last) TRY(cx, emu_allreduce_bf16(cx, hA, (size_t)H, reinterpret_cast<emu_stream_t>(s)));
        }
        ++m->eng_forwards;
        ++m->dl_forwards;
        return 0;
    }

    // ---- one-row step with bf16 weights: whole layers per launch (decode_layer.hip), same bits as the launches of run_launches.  Three
    // schedules (pick_path): layers_per_launch layers in a launch with the all-reduces, if any, inside it; every layer cut at its two
    // all-reduces; or each all-reduce in the tail of the row-sharded projection's launch.
    int run_fused_layers() {
        const LlamaWs& w = ws;
        const emu_stream_t s_ = reinterpret_cast<emu_stream_t>(s);
        DecodeLayersArgs d = plan.dl;
        d.table = m->dl_table; d.hA = hA; d.hB = w.hB; d.qkv = w.qkv; d.attn = w.attn; d.act = w.act; d.ws = w.dec;
        d.cos = m->cos; d.sin = m->sin; d.pos = pos; d.slot = slot; d.kstart = kstart;
        d.kcache = m->kcache; d.vcache = m->vcache; d.kv_layer = kv_layer;
        d.S_max = m->s_max; d.ctx_max = ctx;
        d.eps = eps; d.scale = scale; d.epi_res = epi_res == EPI_RESID ? 1 : 0;
        d.cnt = m->dl_cnt; d.err = m->dl_err;
        d.trace = m->dl_trace;
        if (m->dl_dirty) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            (void)hipStreamIsCapturing(s, &cs);
            if (cs != hipStreamCaptureStatusNone)
                return fail(cx, -16, "emu_llama_forward: the fused decode path needs one eager step before a capture (weight table upload)");
            std::vector<DecodeLayerPtrs> t(m->layers.size());
            for (size_t l = 0; l < t.size(); ++l) { const emu_llama::Layer& L = m->layers[l]; t[l] = {L.qkv.W, L.o.W, L.gu.W, L.down.W, L.ln1, L.ln2}; }
            if (hipStreamSynchronize(s) != hipSuccess ||        // fused launches still in flight on s read the table
                hipMemcpy(m->dl_table, t.data(), sizeof(DecodeLayerPtrs) * t.size(), hipMemcpyHostToDevice) != hipSuccess)
                return fail(cx, -5, "emu_llama_forward: weight table upload");
            m->dl_dirty = false;
        }
        for (int l = m->l0; l < l_end; ++l)
            if (!m->layers[l].qkv.W) return fail(cx, -22, "emu_llama_forward: layer weights not set");
        if (hipMemsetAsync(m->dl_cnt, 0, m->dl_cnt_bytes, s) != hipSuccess) return fail(cx, -5, "emu_llama_forward: hipMemsetAsync");
        if (plan.path == LlamaPath::FusedTailAllReduce) {
            // mode 3: the weight streams with an RMSNorm in front stay stand-alone launches; the attention (split merge by the
            // head's last split) and the two row-sharded projections run as single-role launches whose LAST workgroup to arrive
            // runs the all-reduce -- nobody waits inside a launch except that one workgroup for its peers, so rank processes that
            // share a device cannot starve each other: 5 launches per layer instead of 8
            for (int l = m->l0; l < l_end; ++l) {
                const emu_llama::Layer& L = m->layers[l];
                d.layer0 = l; d.nlayers = 1;
                TRY(cx, project(w, s, hA, L.qkv, nullptr, L.ln1, nullptr, w.qkv, 1, 3 * HD, H, EPI_NONE));
                DecodeLayersArgs a1 = d; a1.tp_n = 0; a1.role0 = 1; a1.role1 = 2;
                TRY(cx, launch_decode_layers(a1, s));
                d.role0 = 2; d.role1 = 3;
                TRY(cx, launch_decode_layers(d, s));
                TRY(cx, project(w, s, w.hB, L.gu, nullptr, L.ln2, nullptr, w.act, 1, 2 * Fl, H, EPI_SWIGLU));
                d.role0 = 4; d.role1 = 5;
                TRY(cx, launch_decode_layers(d, s));
            }
        } else if (plan.path == LlamaPath::FusedCutAtAllReduce) {
            for (int l = m->l0; l < l_end; ++l) {
                d.layer0 = l; d.nlayers = 1;
                d.role0 = 0; d.role1 = 3;
                TRY(cx, launch_decode_layers(d, s));
                TRY(cx, emu_allreduce_bf16(cx, w.hB, (size_t)H, s_));
                d.role0 = 3; d.role1 = 5;
                TRY(cx, launch_decode_layers(d, s));
                TRY(cx, emu_allreduce_bf16(cx, hA, (size_t)H, s_));
            }
        } else {
            const int per = m->dl_per_launch > 0 ? m->dl_per_launch : l_end - m->l0;
            for (int l = m->l0; l < l_end; l += per) {
                d.layer0 = l; d.nlayers = std::min(per, l_end - l);
                TRY(cx, launch_decode_layers(d, s));
            }
        }
        ++m->dl_forwards;
        return 0;
    }
};
}  // namespace

extern "C" {

int emu_llama_create(emu_ctx* ctx, const emu_llama_cfg* cfg, emu_llama** out) {
    if (!ctx || !cfg || !out) return -22;
    if ((cfg->head_dim != 128 && cfg->head_dim != 64) || (cfg->hidden & 7) || (cfg->ffn_local & 7) || cfg->layers < 1)
        return fail(ctx, -22, "emu_llama_create: head_dim must be 64/128, hidden and ffn_local multiples of 8");
    emu_llama* m = new emu_llama();
    m->ctx = ctx; m->cfg = *cfg;
    if (hipMalloc(reinterpret_cast<void**>(&m->arrive), EMU_ARRIVE_INTS * sizeof(int)) != hipSuccess ||
        hipMemset(m->arrive, 0, EMU_ARRIVE_INTS * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        if (m->arrive) (void)hipFree(m->arrive);
        m->arrive = nullptr;                           // the two-launch form needs none
    }
    m->layers.resize(cfg->layers);
    *out = m;
    return 0;
}
void emu_llama_destroy(emu_llama* m) {
    if (m && m->arrive) (void)hipFree(m->arrive);
    if (m && m->dl_table) (void)hipFree(m->dl_table);
    if (m && m->dl_cnt) (void)hipFree(m->dl_cnt);
    if (m && m->dl_err) (void)hipFree(m->dl_err);
    if (m && m->eng_gran) (void)hipFree(m->eng_gran);
    delete m;
}

int emu_llama_set_decode_fused(emu_llama* m, int enable, int layers_per_launch) {
    if (!m || layers_per_launch < 0) return -22;
    if (enable > 0 && m->mode.bf16_released)
        return fail(m->ctx, -22, "emu_llama_set_decode_fused: the bf16 weights were released (emu_llama_release_bf16); the fused decode modes read them");
    if (enable && !m->dl_cnt) {
        const emu_llama_cfg& c = m->cfg;
        m->dl_cnt_bytes = decode_layers_cnt_ints(c.layers, c.heads_local) * sizeof(int);
        if (hipMalloc(reinterpret_cast<void**>(&m->dl_cnt), m->dl_cnt_bytes) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&m->dl_table), sizeof(DecodeLayerPtrs) * c.layers) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&m->dl_err), sizeof(unsigned)) != hipSuccess ||
            hipMemset(m->dl_err, 0, sizeof(unsigned)) != hipSuccess)
            return fail(m->ctx, -12, "emu_llama_set_decode_fused: device allocation");
        m->dl_dirty = true;
    }
    if (enable == 4 && !m->eng_gran) {
        const emu_llama_cfg& c = m->cfg;
        // per layer: the summed post-attention stream (hidden), the SwiGLU product (ffn_local), the summed layer output (hidden)
        m->eng_gran_bytes = (size_t)c.layers * (align_up((size_t)c.hidden * 4) * 2 + align_up((size_t)c.ffn_local * 4));
        if (hipMalloc(reinterpret_cast<void**>(&m->eng_gran), m->eng_gran_bytes) != hipSuccess)
            return fail(m->ctx, -12, "emu_llama_set_decode_fused: device allocation");
    }
    m->decode_fused = enable < 0 ? 0 : (enable > 4 ? 4 : enable);
    m->dl_per_launch = layers_per_launch;
    return 0;
}
int emu_llama_set_decode_trace(emu_llama* m, void* buf) {
    if (!m) return -22;
    m->dl_trace = reinterpret_cast<unsigned long long*>(buf);
    return 0;
}
int emu_llama_decode_fused_stats(emu_llama* m, unsigned int* giveups, long* forwards) {
    if (!m) return -22;
    if (giveups) {
        *giveups = 0;
        if (m->dl_err && hipMemcpy(giveups, m->dl_err, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return -5;
    }
    if (forwards) *forwards = m->dl_forwards;
    return 0;
}

int emu_llama_set_layer(emu_llama* m, int layer, const void* wqkv, const void* wo, const void* wgu, const void* wdown,
                        const void* ln1, const void* ln2) {
    if (!m || layer < 0 || layer >= m->cfg.layers) return -22;
    emu_llama::Layer& L = m->layers[layer];
    L.qkv.W = B(wqkv); L.o.W = B(wo); L.gu.W = B(wgu); L.down.W = B(wdown); L.ln1 = B(ln1); L.ln2 = B(ln2);
    m->dl_dirty = true;
    return 0;
}
int emu_llama_set_layer_fp8(emu_llama* m, int layer, const void* wqkv8, const float* sqkv, const void* wo8, const float* so,
                            const void* wgu8, const float* sgu, const void* wdown8, const float* sdown) {
    if (!m || layer < 0 || layer >= m->cfg.layers) return -22;
    if (!wqkv8 || !sqkv || !wo8 || !so || !wgu8 || !sgu || !wdown8 || !sdown) return -22;
    const emu_llama_cfg& c = m->cfg;
    if ((c.hidden & 15) || ((c.heads_local * c.head_dim) & 15) || (c.ffn_local & 15))
        return fail(m->ctx, -22, "emu_llama_set_layer_fp8: reduction widths must be multiples of 16");
    emu_llama::Layer& L = m->layers[layer];
    L.qkv.W8 = U8(wqkv8); L.o.W8 = U8(wo8); L.gu.W8 = U8(wgu8); L.down.W8 = U8(wdown8);
    L.qkv.s8 = sqkv; L.o.s8 = so; L.gu.s8 = sgu; L.down.s8 = sdown;
    return 0;
}
int emu_llama_set_head_fp8(emu_llama* m, const void* lm_head8, const float* lm_scale) {
    if (!m || !lm_head8 || !lm_scale) return -22;
    m->head.W8 = U8(lm_head8); m->head.s8 = lm_scale;
    return 0;
}
int emu_llama_set_layer_fp4(emu_llama* m, int layer, const void* wqkv4, const void* sqkv, const void* wo4, const void* so,
                            const void* wgu4, const void* sgu, const void* wdown4, const void* sdown) {
    if (!m || layer < 0 || layer >= m->cfg.layers) return -22;
    if (!wqkv4 || !sqkv || !wo4 || !so || !wgu4 || !sgu || !wdown4 || !sdown) return -22;
    emu_llama::Layer& L = m->layers[layer];
    L.qkv.W4 = U8(wqkv4); L.o.W4 = U8(wo4); L.gu.W4 = U8(wgu4); L.down.W4 = U8(wdown4);
    L.qkv.s4 = U8(sqkv); L.o.s4 = U8(so); L.gu.s4 = U8(sgu); L.down.s4 = U8(sdown);
    return 0;
}
int emu_llama_set_head_fp4(emu_llama* m, const void* lm_head4, const void* lm_scales) {
    if (!m || !lm_head4 || !lm_scales) return -22;
    m->head.W4 = U8(lm_head4); m->head.s4 = U8(lm_scales);
    return 0;
}
int emu_llama_use_fp4(emu_llama* m, int enable) {
    if (!m) return -22;
    if (enable < 0 || enable > 3) return fail(m->ctx, -22, "emu_llama_use_fp4: modes 0 to 3");
    if (m->mode.bf16_released && (enable != 3 || m->mode.fp8_all))
        return fail(m->ctx, -22, m->mode.fp8_all ? "emu_llama_use_fp4: the bf16 weights were released under the fp8 set (emu_llama_release_bf16); only fp8 modes 5 / 6 with emu_llama_use_fp8_all run without them"
                                                 : "emu_llama_use_fp4: the bf16 weights were released (emu_llama_release_bf16); only mode 3 runs without them");
    if (enable) {
        const emu_llama_cfg& c = m->cfg;
        if (m->mode.fp8)
            return fail(m->ctx, -22, "emu_llama_use_fp4: the fp8 stream is on; the fp8 and fp4 weight streams are exclusive (emu_llama_use_fp8(m, 0) first)");
        if ((c.hidden & 31) || ((c.heads_local * c.head_dim) & 31) || (c.ffn_local & 31))
            return fail(m->ctx, -22, "emu_llama_use_fp4: reduction widths (hidden, heads_local * head_dim, ffn_local) must be multiples of 32");
        if (!m->head.W4 || std::any_of(m->layers.begin(), m->layers.end(), [](const emu_llama::Layer& l) { return !l.qkv.W4; }))
            return fail(m->ctx, -22, "emu_llama_use_fp4: fp4 weights not set (every layer and the head)");
        if (enable >= 2 && (c.hidden < 256 || c.heads_local * c.head_dim < 256 || c.ffn_local < 256))
            return fail(m->ctx, -22, "emu_llama_use_fp4: modes 2 and 3 (steps of 3 rows and more) need reduction widths (hidden, heads_local * head_dim, ffn_local) of at least 256 that are multiples of 32 (they need not be multiples of 256: the last K stage may be partial)");
    }
    m->mode.fp4 = enable;
    return 0;
}
static int set_pack(emu_llama* m, Weights& w, const emu_bf16_pack_set& s, int N, int K, const char* what) {
    if (!s.rows) { w.pk = PackSet{}; w.pkN = w.pkK = 0; return 0; }       // this matrix stays on bf16
    if (!s.lo || !s.nib || !s.sign || !s.flags || (s.rows != 2 && s.rows != 4) || s.hb < 0 || s.hb > 112 || (K & 31)) return fail(m->ctx, -22, what);
    w.pk = PackSet{};
    w.pk.lo = s.lo; w.pk.nib = s.nib; w.pk.sign = s.sign; w.pk.flags = reinterpret_cast<const uint32_t*>(s.flags); w.pk.hb = s.hb; w.pk.rows = s.rows;
    w.pkN = N; w.pkK = K;
    return 0;
}
static int set_pack12(emu_llama* m, Weights& w, const emu_bf16_pack12_set& s, int N, int K, const char* what) {
    if (!s.rows) { w.pk = PackSet{}; w.pkN = w.pkK = 0; return 0; }       // this matrix stays on bf16
    if (!s.lo || !s.nib || !s.patch || !s.flags || (s.rows != 2 && s.rows != 4) || s.hb < 0 || s.hb > 120 || (K & 31) || (K >> 3) >= PACK12_MAX_KV) return fail(m->ctx, -22, what);
    w.pk = PackSet{};
    w.pk.lo = s.lo; w.pk.nib = s.nib; w.pk.patch = reinterpret_cast<const uint32_t*>(s.patch); w.pk.flags = reinterpret_cast<const uint32_t*>(s.flags);
    w.pk.hb = s.hb; w.pk.rows = s.rows;
    w.pkN = N; w.pkK = K;
    return 0;
}
// the 12-bit setters take a layer's / the head's sets like the 13-bit ones; a matrix whose entry has rows == 0 keeps what it holds
int emu_llama_set_layer_bf16_pack12(emu_llama* m, int layer, const emu_bf16_pack12_set* sets4) {
    if (!m || !sets4 || layer < 0 || layer >= m->cfg.layers) return -22;
    if (m->mode.bf16_released) return fail(m->ctx, -22, "emu_llama_set_layer_bf16_pack12: the bf16 weights were released (emu_llama_release_bf16); flagged row groups read them");
    const emu_llama_cfg& c = m->cfg;
    const int H = c.hidden, HD = c.heads_local * c.head_dim, Fl = c.ffn_local;
    emu_llama::Layer& L = m->layers[layer];
    const char* what = "emu_llama_set_layer_bf16_pack12: a set needs its four pointers, rows 2 or 4, hb 0..120 and K % 32 == 0";
    Weights* ws[4] = {&L.qkv, &L.o, &L.gu, &L.down};
    const int Ns[4] = {3 * HD, H, 2 * Fl, H}, Ks[4] = {H, HD, H, Fl};
    for (int i = 0; i < 4; ++i)
        if (sets4[i].rows)
            if (int st = set_pack12(m, *ws[i], sets4[i], Ns[i], Ks[i], what)) return st;
    return 0;
}
int emu_llama_set_head_bf16_pack12(emu_llama* m, const emu_bf16_pack12_set* set, int rows_n) {
    if (!m || !set || rows_n < 1) return -22;
    if (m->mode.bf16_released) return fail(m->ctx, -22, "emu_llama_set_head_bf16_pack12: the bf16 weights were released (emu_llama_release_bf16); flagged row groups read them");
    return set_pack12(m, m->head, *set, rows_n, m->cfg.hidden, "emu_llama_set_head_bf16_pack12: a set needs its four pointers, rows 2 or 4, hb 0..120 and K % 32 == 0");
}
int emu_llama_set_layer_bf16_pack(emu_llama* m, int layer, const emu_bf16_pack_set* sets4) {
    if (!m || !sets4 || layer < 0 || layer >= m->cfg.layers) return -22;
    if (m->mode.bf16_released) return fail(m->ctx, -22, "emu_llama_set_layer_bf16_pack: the bf16 weights were released (emu_llama_release_bf16); flagged row groups read them");
    const emu_llama_cfg& c = m->cfg;
    const int H = c.hidden, HD = c.heads_local * c.head_dim, Fl = c.ffn_local;
    emu_llama::Layer& L = m->layers[layer];
    const char* what = "emu_llama_set_layer_bf16_pack: a set needs its four pointers, rows 2 or 4, hb 0..112 and K % 32 == 0";
    if (int st = set_pack(m, L.qkv, sets4[0], 3 * HD, H, what)) return st;
    if (int st = set_pack(m, L.o, sets4[1], H, HD, what)) return st;
    if (int st = set_pack(m, L.gu, sets4[2], 2 * Fl, H, what)) return st;
    return set_pack(m, L.down, sets4[3], H, Fl, what);
}
int emu_llama_set_head_bf16_pack(emu_llama* m, const emu_bf16_pack_set* set, int rows_n) {
    if (!m || !set || rows_n < 1) return -22;
    if (m->mode.bf16_released) return fail(m->ctx, -22, "emu_llama_set_head_bf16_pack: the bf16 weights were released (emu_llama_release_bf16); flagged row groups read them");
    return set_pack(m, m->head, *set, rows_n, m->cfg.hidden, "emu_llama_set_head_bf16_pack: a set needs its four pointers, rows 2 or 4, hb 0..112 and K % 32 == 0");
}
int emu_llama_use_bf16_pack(emu_llama* m, int on) {
    if (!m) return -22;
    if (on && m->mode.bf16_released) return fail(m->ctx, -22, "emu_llama_use_bf16_pack: the bf16 weights were released (emu_llama_release_bf16)");
    m->mode.pack = on != 0;
    return 0;
}
int emu_llama_use_bf16_pack_wide(emu_llama* m, int on) {
    if (!m) return -22;
    if (on && m->mode.bf16_released) return fail(m->ctx, -22, "emu_llama_use_bf16_pack_wide: the bf16 weights were released (emu_llama_release_bf16)");
    m->mode.pack_wide = on == 2 ? 2 : on != 0;          // 2: 12-bit sets go to the few-row twin too; 1: 13-bit sets only
    return 0;
}
int emu_llama_release_bf16(emu_llama* m) {
    if (!m) return -22;
    if (m->mode.fp4 != 3 && !(m->mode.fp8 >= 5 && m->mode.fp8_all))
        return fail(m->ctx, -22, "emu_llama_release_bf16: only while emu_llama_use_fp4(m, 3), or emu_llama_use_fp8(m, 5 | 6) with emu_llama_use_fp8_all(m, 1), is on (every row count on the 4-bit / the fp8 set)");
    if (m->decode_fused) return fail(m->ctx, -22, "emu_llama_release_bf16: the fused decode modes read the bf16 weights (emu_llama_set_decode_fused(m, 0, 0) first)");
    for (auto& l : m->layers) {
        l.qkv.W = l.o.W = l.gu.W = l.down.W = nullptr;
        l.qkv.pk = l.o.pk = l.gu.pk = l.down.pk = PackSet{};       // (a flagged row group reads the bf16 rows: the sets go with them)
    }
    m->head.W = nullptr;
    m->head.pk = PackSet{};
    m->mode.pack = m->mode.pack_wide = 0;
    m->dl_dirty = true;
    m->mode.bf16_released = 1;
    return 0;
}
int emu_llama_set_decode_tail(emu_llama* m, int enable) {
    if (!m) return -22;
    m->decode_tail = enable != 0;
    return 0;
}
int emu_llama_set_l2_warm(emu_llama* m, int mask) {
    if (!m || mask < 0 || (mask >> 16)) return -22;
    m->l2_warm = mask;
    return 0;
}
long emu_llama_l2_warm_count(const emu_llama* m) { return m ? m->warm_launches : -1; }
int emu_llama_set_prefill_fusion(emu_llama* m, int enable) {
    if (!m) return -22;
    m->prefill_fusion = enable != 0;
    m->fuse_norm_on = enable != 0;               // sticky part: the K-slice sum + RMSNorm fusion (independent of the slot order)
    return 0;
}
int emu_llama_set_tp_overlap(emu_llama* m, int min_rows) {
    if (!m || min_rows < 0) return -22;
    emu_ctx* cx = m->ctx;
    if (min_rows > 0 && !cx->lane_stream) {                              // created here, never inside a forward (stream capture)
        if (hipSetDevice(cx->device) != hipSuccess) return fail(cx, -19, "emu_llama_set_tp_overlap: hipSetDevice");
        if (hipStreamCreateWithFlags(&cx->lane_stream, hipStreamNonBlocking) != hipSuccess) {
            cx->lane_stream = nullptr;
            return fail(cx, -12, "emu_llama_set_tp_overlap: hipStreamCreateWithFlags");
        }
        for (hipEvent_t& e : cx->ar_ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
                e = nullptr;
                return fail(cx, -12, "emu_llama_set_tp_overlap: hipEventCreateWithFlags");
            }
    }
    m->tp_overlap_rows = min_rows > 0 && min_rows < 512 ? 512 : min_rows;   // two halves of at least one 256-row tile each
    return 0;
}
long emu_llama_tp_overlap_count(const emu_llama* m) { return m ? m->ov_forwards : -1; }
int emu_llama_use_fp8(emu_llama* m, int enable) {
    if (!m) return -22;
    if (enable < 0 || enable > 6) return fail(m->ctx, -22, "emu_llama_use_fp8: modes 0 to 6");
    if (m->mode.bf16_released && (m->mode.fp8_all ? enable < 5 : enable != 0))
        return fail(m->ctx, -22, m->mode.fp8_all ? "emu_llama_use_fp8: the bf16 weights were released (emu_llama_release_bf16); only modes 5 and 6 with emu_llama_use_fp8_all run without them"
                                                 : "emu_llama_use_fp8: the bf16 weights were released (emu_llama_release_bf16); only the fp4 mode 3 runs without them");
    if (enable && m->mode.fp4)
        return fail(m->ctx, -22, "emu_llama_use_fp8: the fp4 stream is on; the fp8 and fp4 weight streams are exclusive (emu_llama_use_fp4(m, 0) first)");
    // (emu_llama_set_layer_fp8 was never called: it sets all of a layer's or refuses, and a model has at least one layer)
    if (enable && std::none_of(m->layers.begin(), m->layers.end(), [](const emu_llama::Layer& l) { return l.qkv.W8; }))
        return fail(m->ctx, -22, "emu_llama_use_fp8: fp8 layer weights not set");
    if (enable >= 3) {
        const emu_llama_cfg& c = m->cfg;
        if ((c.hidden & 255) || ((c.heads_local * c.head_dim) & 255) || (c.ffn_local & 255))
            return fail(m->ctx, -22, "emu_llama_use_fp8: modes 3 to 6 (steps of 3..16 / 17..64 rows on the fp8 set) need reduction widths (hidden, heads_local * head_dim, ffn_local) that are multiples of 256");
        if (std::any_of(m->layers.begin(), m->layers.end(), [](const emu_llama::Layer& l) { return !l.qkv.W8; }))
            return fail(m->ctx, -22, "emu_llama_use_fp8: modes 3 to 6 need the fp8 weights of every layer");
    }
    m->mode.fp8 = enable;
    if (enable < 5) m->mode.fp8_all = 0;         // the switch lives beside modes 5 / 6 only
    return 0;
}
int emu_llama_use_fp8_all(emu_llama* m, int on) {
    if (!m) return -22;
    if (on != 0 && on != 1) return fail(m->ctx, -22, "emu_llama_use_fp8_all: 0 or 1");
    if (!on && m->mode.bf16_released && m->mode.fp8_all)
        return fail(m->ctx, -22, "emu_llama_use_fp8_all: the bf16 weights were released (emu_llama_release_bf16); the switch is pinned");
    if (on) {
        if (m->mode.fp4) return fail(m->ctx, -22, "emu_llama_use_fp8_all: the fp4 stream is on; the fp8 and fp4 weight streams are exclusive");
        if (m->mode.fp8 < 5) return fail(m->ctx, -22, "emu_llama_use_fp8_all: needs emu_llama_use_fp8(m, 5 | 6) (every row count below 65 on the fp8 set)");
        if (!m->head.W8 || !m->head.s8) return fail(m->ctx, -22, "emu_llama_use_fp8_all: the head's fp8 copy is not set (emu_llama_set_head_fp8)");
    }
    m->mode.fp8_all = on;
    return 0;
}
int emu_llama_set_head(emu_llama* m, const void* final_norm, const void* lm_head, const void* embed, const void* rope_cos,
                       const void* rope_sin) {
    if (!m) return -22;
    m->final_norm = B(final_norm); m->head.W = B(lm_head); m->embed = B(embed); m->cos = B(rope_cos); m->sin = B(rope_sin);
    return 0;
}
int emu_llama_set_head_shard(emu_llama* m, int row0, int rows) {
    if (!m) return -22;
    if (rows < 0) { m->head_row0 = 0; m->head_rows = -1; return 0; }
    if (row0 < 0 || rows < 1 || row0 + rows > m->cfg.vocab) return fail(m->ctx, -22, "emu_llama_set_head_shard: rows outside the vocabulary");
    m->head_row0 = row0; m->head_rows = rows;
    return 0;
}
int emu_llama_set_kv(emu_llama* m, void* kcache, void* vcache, int batch, int s_max) {
    if (!m) return -22;
    if (!kcache && !vcache) {                    // detach: the caller freed the caches; every later forward fails with -22 until new ones are set
        m->kcache = m->vcache = nullptr; m->kv_batch = m->s_max = 0;
        m->kv_share_nb = m->kv_share_len = 0;
        m->kprefix = m->vprefix = nullptr; m->prefix_s_max = m->prefix_len = 0;
        return 0;
    }
    if (!kcache || !vcache || batch < 1 || s_max < 1) return -22;
    m->kcache = B(kcache); m->vcache = B(vcache); m->kv_batch = batch; m->s_max = s_max;
    m->kv_share_nb = m->kv_share_len = 0;
    m->kprefix = m->vprefix = nullptr; m->prefix_s_max = m->prefix_len = 0;
    return 0;
}
int emu_llama_set_kv_prefix(emu_llama* m, const void* kprefix, const void* vprefix, int prefix_s_max, int prefix_len) {
    if (!m) return -22;
    if (!kprefix || !vprefix || prefix_len == 0) { m->kprefix = m->vprefix = nullptr; m->prefix_s_max = m->prefix_len = 0; return 0; }
    if (prefix_len < 0 || prefix_len > prefix_s_max) return fail(m->ctx, -22, "emu_llama_set_kv_prefix: prefix_len within the prefix caches' capacity");
    if (m->cfg.head_dim != 128) return fail(m->ctx, -22, "emu_llama_set_kv_prefix: the two-segment attention has head_dim 128 only");
    if (!m->kcache) return fail(m->ctx, -22, "emu_llama_set_kv_prefix: set the rows' own cache first (emu_llama_set_kv)");
    if (m->kv_share_nb > 1) return fail(m->ctx, -22, "emu_llama_set_kv_prefix: not together with emu_llama_set_kv_share");
    m->kprefix = B(kprefix); m->vprefix = B(vprefix); m->prefix_s_max = prefix_s_max; m->prefix_len = prefix_len;
    return 0;
}
int emu_llama_set_kv_share(emu_llama* m, int beams, int shared_slots) {
    if (!m) return -22;
    if (beams <= 1) { m->kv_share_nb = m->kv_share_len = 0; return 0; }
    if (m->prefix_len > 0) return fail(m->ctx, -22, "emu_llama_set_kv_share: not while a KV prefix is set (emu_llama_set_kv_prefix)");
    if (beams > DECODE_SHARE_MAX || !m->kcache || m->kv_batch % beams || shared_slots < 0 || shared_slots > m->s_max)
        return fail(m->ctx, -22, "emu_llama_set_kv_share: 2..8 beams dividing the cache batch, shared slots within the capacity");
    m->kv_share_nb = beams; m->kv_share_len = shared_slots;
    return 0;
}
int emu_llama_set_layer_range(emu_llama* m, int l0, int l1) {
    if (!m || l0 < 0 || l1 > m->cfg.layers || (l1 >= 0 && l1 < l0)) return -22;
    m->l0 = l0; m->l1 = l1;
    return 0;
}
size_t emu_llama_workspace_bytes(const emu_llama* m, int Bn, int T) {
    if (!m) return 0;
    return llama_ws(m, Bn, T, nullptr).total;
}

int emu_llama_forward(emu_llama* m, void* hidden, int Bn, int T, const int32_t* pos, const int32_t* slot,
                      const int32_t* kstart, const int32_t* ctx_dev, int ctx, void* workspace, size_t ws_bytes,
                      emu_stream_t s_) {
    if (!m) return -22;
    // the slot-order promise (emu_llama_set_prefill_fusion) is per call: every T > 1 entry consumes it, whatever happens below -- an
    // early return must not leave it armed for an unrelated caller
    const bool promise = m->prefill_fusion;
    if (T > 1) m->prefill_fusion = false;
    if (!hidden || !pos || !slot) return -22;
    emu_ctx* cx = m->ctx;
    const emu_llama_cfg& c = m->cfg;
    if (!m->kcache || Bn != m->kv_batch) return fail(cx, -22, "emu_llama_forward: KV cache not set for this batch size");
    if (ctx < 1 || ctx > m->s_max) return fail(cx, -22, "emu_llama_forward: ctx out of range");
    if (!m->cos) return fail(cx, -22, "emu_llama_forward: rope tables not set");
    if (m->prefix_len > 0) {                     // every refusal of the two-segment form, before any launch
        if (T == 1) return fail(cx, -22, "emu_llama_forward: a KV prefix serves T > 1 rows only (emu_llama_set_kv_prefix(m, NULL, NULL, 0, 0) first)");
        if (m->kv_share_nb > 1) return fail(cx, -22, "emu_llama_forward: a KV prefix and emu_llama_set_kv_share exclude each other");
        if (m->decode_fused) return fail(cx, -22, "emu_llama_forward: a KV prefix and the fused decode modes exclude each other");
        if (m->tp_overlap_rows > 0) return fail(cx, -22, "emu_llama_forward: a KV prefix has no two-lane tensor-parallel prefill (emu_llama_set_tp_overlap(m, 0) first)");
        if (c.head_dim != 128) return fail(cx, -22, "emu_llama_forward: a KV prefix needs head_dim 128");
    }
    LlamaCall f{};
    f.m = m; f.cx = cx; f.ws = llama_ws(m, Bn, T, workspace);
    if (f.ws.total > ws_bytes) return fail(cx, -12, "emu_llama_forward: workspace too small");
    f.hA = B(hidden); f.pos = pos; f.slot = slot; f.kstart = kstart; f.s = S(s_);
    f.Bn = Bn; f.T = T; f.M = Bn * T; f.ctx = ctx; f.spad = (ctx + 63) / 64 * 64; f.l_end = m->l1 < 0 ? c.layers : m->l1;
    f.H = c.hidden; f.Hl = c.heads_local; f.D = c.head_dim; f.HD = f.Hl * f.D; f.Fl = c.ffn_local;
    f.tp = cx->tp_size > 1 || cx->comm != nullptr || cx->p2p_on;
    f.epi_res = (!f.tp || cx->tp_rank == 0) ? EPI_RESID : EPI_NONE;
    f.scale = 1.0f / sqrtf((float)f.D); f.eps = c.rms_eps; f.kv_layer = (size_t)Bn * f.Hl * m->s_max * f.D;
    f.pick_path(promise);
    // The V^T buffer's pad columns [ctx, spad) are never written by the qkv epilogue: zeroed once per call (the attention kernel
    // multiplies them by masked probabilities).
    if (f.plan.fuse_rope && hipMemsetAsync(f.ws.vt, 0, (size_t)f.HD * f.spad * 2, f.s) != hipSuccess) return fail(cx, -5, "emu_llama_forward: hipMemsetAsync");
    switch (f.plan.path) {
    case LlamaPath::Engine: return f.run_engine();
    case LlamaPath::TwoLane: return f.llama_prefill_overlapped();
    case LlamaPath::Launches: return f.run_launches();
    case LlamaPath::FusedLayers: case LlamaPath::FusedCutAtAllReduce: case LlamaPath::FusedTailAllReduce: return f.run_fused_layers();
    }
    return -22;                                  // (not reached: every path returns above)
}

size_t emu_llama_chunk_workspace_bytes(const emu_llama* m, int Bn, int T) {
    if (!m) return 0;
    return llama_ws(m, Bn, T, nullptr, true).total;
}

int emu_llama_forward_chunk(emu_llama* m, void* hidden, int Bn, int T, const int32_t* pos0, const int32_t* slot0, const int32_t* kstart,
                            const int32_t* ctx_dev, int ctx_upper, void* workspace, size_t ws_bytes, emu_stream_t s_) {
    (void)ctx_dev;                               // (every row's context follows from slot0 on the device; kept for the callers' symmetry)
    if (!m || !hidden || !pos0 || !slot0) return -22;
    emu_ctx* cx = m->ctx;
    const emu_llama_cfg& c = m->cfg;
    if (T < 2 || T > DECODE_CHUNK_MAX || Bn < 1 || Bn * T > 16) return fail(cx, -22, "emu_llama_forward_chunk: T in 2..8 and B * T <= 16");
    if (cx->tp_size > 1 || cx->comm != nullptr || cx->p2p_on) return fail(cx, -22, "emu_llama_forward_chunk: no tensor-parallel form");
    if (m->kv_share_nb > 1) return fail(cx, -22, "emu_llama_forward_chunk: shared-prefix KV rows serve single-token steps only");
    if (m->prefix_len > 0) return fail(cx, -22, "emu_llama_forward_chunk: a KV prefix serves emu_llama_forward with T > 1 only");
    if (m->decode_fused) return fail(cx, -22, "emu_llama_forward_chunk: the fused decode modes 1-4 are one-row steps (emu_llama_set_decode_fused(m, 0, 0) first)");
    if (!m->kcache || Bn != m->kv_batch) return fail(cx, -22, "emu_llama_forward_chunk: KV cache not set for this batch size");
    if (ctx_upper < 1 || ctx_upper > m->s_max) return fail(cx, -22, "emu_llama_forward_chunk: ctx out of range");
    if (!m->cos) return fail(cx, -22, "emu_llama_forward_chunk: rope tables not set");
    LlamaCall f{};
    f.m = m; f.cx = cx; f.ws = llama_ws(m, Bn, T, workspace, true);
    if (f.ws.total > ws_bytes) return fail(cx, -12, "emu_llama_forward_chunk: workspace too small");
    f.hA = B(hidden); f.pos = pos0; f.slot = slot0; f.kstart = kstart; f.s = S(s_);
    f.Bn = Bn; f.T = T; f.M = Bn * T; f.ctx = ctx_upper; f.spad = (ctx_upper + 63) / 64 * 64; f.l_end = m->l1 < 0 ? c.layers : m->l1;
    f.H = c.hidden; f.Hl = c.heads_local; f.D = c.head_dim; f.HD = f.Hl * f.D; f.Fl = c.ffn_local;
    f.tp = false; f.epi_res = EPI_RESID;
    f.scale = 1.0f / sqrtf((float)f.D); f.eps = c.rms_eps; f.kv_layer = (size_t)Bn * f.Hl * m->s_max * f.D;
    f.chunk = true;
    f.plan_chunk();
    return f.run_launches();
}

size_t emu_beam_step_workspace_bytes(int Bn, int nb, int V) { return beam_step_ws_floats(Bn, nb, V) * sizeof(float); }
int emu_beam_step_bf16(const void* logits, long ld_prompt, long ld_beam, int V, int Bn, int nb, int L, int cur, const int32_t* cur_dev,
                       int min_len, int eos_id, float length_penalty, int hf431, int32_t* running_seq, int32_t* sequences, float* running_scores, float* beam_scores,
                       unsigned char* finished, int32_t* seq_len, unsigned char* heuristic_open, int32_t* next_tok, long* beam_flat,
                       void* workspace, size_t ws_bytes, emu_stream_t s) {
    if (!logits || !running_seq || !sequences || !running_scores || !beam_scores || !finished || !seq_len || !heuristic_open ||
        !next_tok || !beam_flat)
        return -22;
    BeamStepArgs a{B(logits), ld_prompt, ld_beam, V, Bn, nb, L, cur, cur_dev, min_len, eos_id, length_penalty, hf431, running_seq, sequences,
                   running_scores, beam_scores, finished, seq_len, heuristic_open, next_tok, beam_flat};
    return launch_beam_step(a, reinterpret_cast<float*>(workspace), ws_bytes / sizeof(float), S(s));
}
int emu_beam_step_ngram_bf16(const void* logits, long ld_prompt, long ld_beam, int V, int Bn, int nb, int L, int cur, const int32_t* cur_dev,
                             int min_len, int eos_id, float length_penalty, int hf431, int32_t* running_seq, int32_t* sequences,
                             float* running_scores, float* beam_scores, unsigned char* finished, int32_t* seq_len,
                             unsigned char* heuristic_open, int32_t* next_tok, long* beam_flat, void* workspace, size_t ws_bytes,
                             int ngram, emu_stream_t s) {
    if (!logits || !running_seq || !sequences || !running_scores || !beam_scores || !finished || !seq_len || !heuristic_open ||
        !next_tok || !beam_flat || ngram < 0)
        return -22;
    BeamStepArgs a{B(logits), ld_prompt, ld_beam, V, Bn, nb, L, cur, cur_dev, min_len, eos_id, length_penalty, hf431, running_seq, sequences,
                   running_scores, beam_scores, finished, seq_len, heuristic_open, next_tok, beam_flat};
    a.ngram = ngram;
    return launch_beam_step(a, reinterpret_cast<float*>(workspace), ws_bytes / sizeof(float), S(s));
}
int emu_beam_step_trie_bf16(const void* logits, long ld_prompt, long ld_beam, int V, int Bn, int nb, int L, int cur, const int32_t* cur_dev,
                            int min_len, int eos_id, float length_penalty, int hf431, int32_t* running_seq, int32_t* sequences,
                            float* running_scores, float* beam_scores, unsigned char* finished, int32_t* seq_len,
                            unsigned char* heuristic_open, int32_t* next_tok, long* beam_flat, void* workspace, size_t ws_bytes,
                            const emu_token_trie* trie, int32_t* node, emu_stream_t s) {
    if (!logits || !running_seq || !sequences || !running_scores || !beam_scores || !finished || !seq_len || !heuristic_open ||
        !next_tok || !beam_flat || !trie || !node)
        return -22;
    BeamStepArgs a{B(logits), ld_prompt, ld_beam, V, Bn, nb, L, cur, cur_dev, min_len, eos_id, length_penalty, hf431, running_seq, sequences,
                   running_scores, beam_scores, finished, seq_len, heuristic_open, next_tok, beam_flat, *trie, node};
    return launch_beam_step(a, reinterpret_cast<float*>(workspace), ws_bytes / sizeof(float), S(s));
}

size_t emu_beam_sample_workspace_bytes(int Bn, int nb, int V) { return beam_sample_ws_floats(Bn, nb, V) * sizeof(float); }
int emu_beam_sample_step_ngram_bf16(const void* logits, long ld_prompt, long ld_beam, int V, int Bn, int nb, int L, int cur,
                                    const int32_t* cur_dev, int min_len, int eos_id, float length_penalty, int hf431, int32_t* running_seq,
                                    int32_t* sequences, float* running_scores, float* beam_scores, unsigned char* finished,
                                    int32_t* seq_len, unsigned char* heuristic_open, int32_t* next_tok, long* beam_flat, void* workspace,
                                    size_t ws_bytes, const emu_sample_params* params, int warp_accumulated, const float* uniforms,
                                    int uni_rows, int32_t* draws_out, float* acc_out, long ld_acc, int ngram, emu_stream_t s) {
    if (!logits || !running_seq || !sequences || !running_scores || !beam_scores || !finished || !seq_len || !heuristic_open ||
        !next_tok || !beam_flat || !params || ngram < 0)
        return -22;
    BeamSampleArgs a;
    a.st = BeamStepArgs{B(logits), ld_prompt, ld_beam, V, Bn, nb, L, cur, cur_dev, min_len, eos_id, length_penalty, hf431, running_seq,
                        sequences, running_scores, beam_scores, finished, seq_len, heuristic_open, next_tok, beam_flat};
    a.st.ngram = ngram;
    a.penalty = params->repetition_penalty;
    a.do_sample = params->do_sample; a.temperature = params->temperature; a.top_k = params->top_k; a.top_p = params->top_p;
    a.min_keep = params->min_keep < 2 ? 2 : params->min_keep;      // the library's warpers under beam search: one EOS id + 1
    a.warp_accumulated = warp_accumulated;
    a.uniforms = uniforms; a.uni_rows = uni_rows;
    a.draws_out = draws_out; a.acc_out = acc_out; a.ld_acc = ld_acc;
    return launch_beam_sample_step(a, reinterpret_cast<float*>(workspace), ws_bytes / sizeof(float), S(s));
}
int emu_beam_sample_step_bf16(const void* logits, long ld_prompt, long ld_beam, int V, int Bn, int nb, int L, int cur, const int32_t* cur_dev,
                              int min_len, int eos_id, float length_penalty, int hf431, int32_t* running_seq, int32_t* sequences,
                              float* running_scores, float* beam_scores, unsigned char* finished, int32_t* seq_len,
                              unsigned char* heuristic_open, int32_t* next_tok, long* beam_flat, void* workspace, size_t ws_bytes,
                              const emu_sample_params* params, int warp_accumulated, const float* uniforms, int uni_rows,
                              int32_t* draws_out, float* acc_out, long ld_acc, emu_stream_t s) {
    return emu_beam_sample_step_ngram_bf16(logits, ld_prompt, ld_beam, V, Bn, nb, L, cur, cur_dev, min_len, eos_id, length_penalty, hf431,
                                           running_seq, sequences, running_scores, beam_scores, finished, seq_len, heuristic_open,
                                           next_tok, beam_flat, workspace, ws_bytes, params, warp_accumulated, uniforms, uni_rows,
                                           draws_out, acc_out, ld_acc, 0, s);
}

int emu_regress_advance_bf16(const void* src, void* out_all, void* prev, int32_t* pos, int32_t* slot, int32_t* step_dev, int Bn,
                             int cols, emu_stream_t s) {
    if (!src || !out_all || !prev || !pos || !slot || !step_dev) return -22;
    return launch_regress_advance(B(src), B(out_all), B(prev), pos, slot, step_dev, Bn, cols, S(s));
}
int emu_beam_advance(int32_t* cur_dev, int32_t* pos, int32_t* slot, const int32_t* pos0, int slot0, int rows, int L, int phase,
                     emu_stream_t s) {
    return launch_step_advance(cur_dev, pos, slot, pos0, slot0, -1, rows, L, phase, S(s));
}
int emu_llama_beam_reorder_kv(emu_llama* m, const long* beam_flat, const int32_t* cur_dev, int beams, int slot0, int L,
                              emu_stream_t s) {
    if (!m || !m->kcache) return -22;
    return launch_beam_reorder(m->kcache, m->vcache, beam_flat, cur_dev, m->cfg.layers, m->kv_batch, m->cfg.heads_local, m->s_max,
                               m->cfg.head_dim, beams, slot0, L, S(s));
}

int emu_llama_contrastive_keep_kv(emu_llama* m, const int32_t* sel, const int32_t* step_dev, int k, int slot0, int L, emu_stream_t s) {
    if (!m || !m->kcache) return -22;
    return launch_contrastive_keep(m->kcache, m->vcache, sel, step_dev, m->cfg.layers, m->kv_batch, m->cfg.heads_local, m->s_max,
                                   m->cfg.head_dim, k, slot0, L, S(s));
}
int emu_contrastive_pick_bf16(const void* logits, int ld, int V, int Bn, int k, int L, const int32_t* sel, const int32_t* hist, int hist_ld,
                              const int32_t* step_dev, float repetition_penalty, int eos_id, int min_len, int32_t* cand_ids,
                              float* cand_p, emu_stream_t s) {
    ContrastivePickArgs a{B(logits), ld, V, Bn, k, L, sel, hist, hist_ld, step_dev, repetition_penalty, eos_id, min_len, cand_ids, cand_p};
    return launch_contrastive_pick(a, S(s));
}
size_t emu_contrastive_workspace_bytes(int Bn, int k, int Lc) { return contrastive_ws_floats(Bn, k, Lc) * sizeof(float); }
int emu_contrastive_score(float* ctx_n, const void* cand, const int32_t* cand_ids, const float* cand_p, const int32_t* kstart,
                          const int32_t* step_dev, int Bn, int k, int H, int S_, int L, int Lc, float alpha, float one_minus_alpha,
                          int eos_id, int pad_id, int32_t* out_ids, int32_t* unfinished, int32_t* sel, float* pen_out, void* workspace,
                          size_t ws_bytes, emu_stream_t s) {
    ContrastiveScoreArgs a{ctx_n, B(cand), cand_ids, cand_p, kstart, step_dev, Bn, k, H, S_, L, Lc, alpha, one_minus_alpha, eos_id, pad_id,
                           out_ids, unfinished, sel, pen_out, reinterpret_cast<float*>(workspace), 0};
    return launch_contrastive_score(a, ws_bytes / sizeof(float), S(s));
}
int emu_contrastive_advance(int32_t* step_dev, int32_t* pos, int32_t* slot, const int32_t* pos0, int slot0, int rows, int L, int phase,
                            emu_stream_t s) {
    return launch_step_advance(step_dev, pos, slot, pos0, slot0, 0, rows, L, phase, S(s));
}

int emu_llama_final_norm(emu_llama* m, const void* hidden, void* out, int rows, emu_stream_t s) {
    if (!m || !m->final_norm) return -22;
    return launch_rmsnorm(B(hidden), m->final_norm, B(out), rows, m->cfg.hidden, m->cfg.hidden, m->cfg.hidden,
                          m->cfg.rms_eps, S(s));
}

// final RMSNorm + rows of the head (N of them, from the engine's head record) on M hidden rows -> out.  The kernel, and whether
// the norm rides in its stream or is a launch into the workspace first, is matrix_kernel's answer for the head site.
static int llama_head(emu_llama* m, const bf16_t* hidden, int ldh, int M, bf16_t* out, int N, int ld, bf16_t* ws, size_t ws_bytes,
                      hipStream_t s) {
    const emu_llama_cfg& c = m->cfg;
    const int H = c.hidden;
    const bool ws_fits = ws_bytes >= (size_t)M * H * 2;
    // (the tail and warm switches as set; a layer projection passes what its call's plan made of them: kept as found, it looks accidental)
    emu_projection q = m->site(m->head, M, N, H, true, EPI_NONE, m->decode_tail, m->l2_warm);
    q.head = 1; q.ws_fits = ws_fits;
    const WeightKernel k = matrix_kernel(m->kernel_for(M), q);
    const bool fused = q.norm_in_stream != 0;
    if (!fused) {
        if (!ws_fits) return fail(m->ctx, -12, "emu_llama_logits: workspace too small");
        TRY(m->ctx, launch_rmsnorm(hidden, m->final_norm, ws, M, H, ldh, H, c.rms_eps, s));
    }
    return linear_w(k, m->head, packed(k, fused ? hidden : ws, fused ? ldh : H, fused ? m->final_norm : nullptr, c.rms_eps, nullptr, 0, out, ld,
                                       M, N, H, EPI_NONE), s, nullptr, 0, m->mode.pack_wide);
}

int emu_llama_logits(emu_llama* m, const void* hidden, int ldh, int M, void* logits, int ld, void* workspace,
                     size_t ws_bytes, emu_stream_t s) {
    if (!m || !m->final_norm) return -22;
    // after emu_llama_release_bf16 the 4-bit head (mode 3 pinned) or the fp8 head (modes 5 / 6 with fp8_all pinned) is the head: every
    // row count has a path on it in llama_head
    if (m->mode.bf16_released ? (m->mode.fp8_all ? m->mode.fp8 < 5 || !m->head.W8 : m->mode.fp4 != 3 || !m->head.W4) : !m->head.W) return -22;
    const emu_llama_cfg& c = m->cfg;
    if (m->head_rows < 0) return llama_head(m, B(hidden), ldh, M, B(logits), c.vocab, ld, B(workspace), ws_bytes, S(s));
    // vocabulary-sharded head (tensor parallelism): this rank streams its rows of lm_head only (4035 of 32 274 at TP = 8:
    // 54 MB instead of 430 MB per token) into its own columns of the caller's [M, vocab] rows, every other column zero, and one
    // all-reduce makes the rows whole on every rank -- each logit is computed by exactly one rank and summed with zeros, so the
    // result is bit-identical to the replicated head and every consumer (arg-max, beam scorer, samplers) stays as it is.
    emu_ctx* cx = m->ctx;
    bf16_t* lg = B(logits);
    if (hipMemsetAsync(lg, 0, ((size_t)(M - 1) * ld + c.vocab) * sizeof(bf16_t), S(s)) != hipSuccess)
        return fail(cx, -5, "emu_llama_logits: hipMemsetAsync");
    TRY(cx, llama_head(m, B(hidden), ldh, M, lg + m->head_row0, m->head_rows, ld, B(workspace), ws_bytes, S(s)));
    if (ld == c.vocab) return emu_allreduce_bf16(cx, lg, (size_t)M * c.vocab, s);
    for (int r = 0; r < M; ++r) TRY(cx, emu_allreduce_bf16(cx, lg + (size_t)r * ld, (size_t)c.vocab, s));
    return 0;
}

// One token of the greedy, the sampling and the teacher-forced loop: embed -> layers -> logits -> select -> state advance.  The
// selection is the only difference: `score` set = the token is FORCED (targets[step, :] of score->T rows, its log-probability under
// the logits filed at [step, :]; nothing is selected, filed or advanced once step >= T); else `params` null = arg-max; else
// emu_sample_bf16's kernel, for which the ids of steps 0 .. step - 1 in out_ids are the history (with `trie` and `node`:
// emu_sample_trie_bf16's, the rows' trie nodes advancing on the device; with `ngram` > 0: emu_sample_ngram_bf16's, the no-repeat
// n-gram ban over the same history).  Either way the selection goes to
// cur_ids and the advance files it at `step` (the forced loop has no out_ids: its tokens are the caller's).
struct ScoreSel { const int32_t* targets; int T; float* lp; float* lse; int32_t* top1; };
static int llama_token_step(emu_llama* m, int Bn, int32_t* cur_ids, int32_t* pos, int32_t* slot, const int32_t* kstart, int32_t* ctx_dev,
                            int32_t* step_dev, int32_t* out_ids, int max_new, int ctx_upper, void* hidden, void* logits, int ld_logits,
                            void* workspace, size_t ws_bytes, const float* uniforms, int32_t* unfinished,
                            const emu_sample_params* params, const ScoreSel* score, const emu_token_trie* trie, int32_t* node,
                            int ngram, emu_stream_t s) {
    const emu_llama_cfg& c = m->cfg;
    if (m->prefix_len > 0) return fail(m->ctx, -22, "token step: a KV prefix serves emu_llama_forward with T > 1 only");   // before the first launch
    TRY(m->ctx, launch_embed_gather(cur_ids, m->embed, B(hidden), Bn, c.hidden, c.vocab, S(s)));
    TRY(m->ctx, emu_llama_forward(m, hidden, Bn, 1, pos, slot, kstart, ctx_dev, ctx_upper, workspace, ws_bytes, s));
    TRY(m->ctx, emu_llama_logits(m, hidden, c.hidden, Bn, logits, ld_logits, workspace, ws_bytes, s));
    if (score) TRY(m->ctx, launch_token_logprob(B(logits), ld_logits, Bn, c.vocab, score->targets, Bn, step_dev, score->T, nullptr, 0,
                                                score->lp, score->lse, score->top1, nullptr, nullptr, Bn, cur_ids, S(s)));
    else if (!params) TRY(m->ctx, launch_argmax(B(logits), ld_logits, Bn, c.vocab, -1, cur_ids, S(s)));
    else TRY(m->ctx, launch_sample(B(logits), ld_logits, Bn, c.vocab, out_ids, Bn, max_new, step_dev, uniforms, Bn, max_new, params,
                                   unfinished, cur_ids, nullptr, 0, trie, node, ngram, S(s)));
    TRY(m->ctx, launch_greedy_advance(cur_ids, pos, slot, ctx_dev, step_dev, out_ids, Bn, score ? score->T : 0, S(s)));
    return 0;
}

int emu_llama_greedy_step(emu_llama* m, int Bn, int32_t* cur_ids, int32_t* pos, int32_t* slot, const int32_t* kstart,
                          int32_t* ctx_dev, int32_t* step_dev, int32_t* out_ids, int ctx_upper, void* hidden,
                          void* logits, int ld_logits, void* workspace, size_t ws_bytes, emu_stream_t s) {
    if (!m || !m->embed) return -22;
    return llama_token_step(m, Bn, cur_ids, pos, slot, kstart, ctx_dev, step_dev, out_ids, 0, ctx_upper, hidden, logits, ld_logits,
                            workspace, ws_bytes, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, s);
}

int emu_llama_sample_step(emu_llama* m, int Bn, int32_t* cur_ids, int32_t* pos, int32_t* slot, const int32_t* kstart,
                          int32_t* ctx_dev, int32_t* step_dev, int32_t* out_ids, int max_new, int ctx_upper, void* hidden,
                          void* logits, int ld_logits, void* workspace, size_t ws_bytes, const float* uniforms,
                          int32_t* unfinished, const emu_sample_params* params, emu_stream_t s) {
    if (!m || !m->embed || !params || !unfinished || max_new < 1) return -22;
    if (m->cfg.vocab > EMU_SAMPLE_MAX_VOCAB) return -22;           // refused before anything is launched
    return llama_token_step(m, Bn, cur_ids, pos, slot, kstart, ctx_dev, step_dev, out_ids, max_new, ctx_upper, hidden, logits, ld_logits,
                            workspace, ws_bytes, uniforms, unfinished, params, nullptr, nullptr, nullptr, 0, s);
}

int emu_llama_sample_step_ngram(emu_llama* m, int Bn, int32_t* cur_ids, int32_t* pos, int32_t* slot, const int32_t* kstart,
                                int32_t* ctx_dev, int32_t* step_dev, int32_t* out_ids, int max_new, int ctx_upper, void* hidden,
                                void* logits, int ld_logits, void* workspace, size_t ws_bytes, const float* uniforms,
                                int32_t* unfinished, const emu_sample_params* params, int ngram, emu_stream_t s) {
    if (!m || !m->embed || !params || !unfinished || max_new < 1 || ngram < 0) return -22;
    if (m->cfg.vocab > EMU_SAMPLE_MAX_VOCAB) return -22;           // refused before anything is launched
    return llama_token_step(m, Bn, cur_ids, pos, slot, kstart, ctx_dev, step_dev, out_ids, max_new, ctx_upper, hidden, logits, ld_logits,
                            workspace, ws_bytes, uniforms, unfinished, params, nullptr, nullptr, nullptr, ngram, s);
}

int emu_llama_sample_step_trie(emu_llama* m, int Bn, int32_t* cur_ids, int32_t* pos, int32_t* slot, const int32_t* kstart,
                               int32_t* ctx_dev, int32_t* step_dev, int32_t* out_ids, int max_new, int ctx_upper, void* hidden,
                               void* logits, int ld_logits, void* workspace, size_t ws_bytes, const float* uniforms,
                               int32_t* unfinished, const emu_sample_params* params, const emu_token_trie* trie, int32_t* node,
                               emu_stream_t s) {
    if (!m || !m->embed || !params || !unfinished || max_new < 1) return -22;
    if (m->cfg.vocab > EMU_SAMPLE_MAX_VOCAB) return -22;           // refused before anything is launched
    if (!trie || !node || !trie->first || trie->nodes < 1 || trie->edges < 0 || (trie->edges > 0 && (!trie->tok || !trie->child)))
        return -22;
    return llama_token_step(m, Bn, cur_ids, pos, slot, kstart, ctx_dev, step_dev, out_ids, max_new, ctx_upper, hidden, logits, ld_logits,
                            workspace, ws_bytes, uniforms, unfinished, params, nullptr, trie, node, 0, s);
}

int emu_llama_score_step(emu_llama* m, int Bn, int32_t* cur_ids, int32_t* pos, int32_t* slot, const int32_t* kstart,
                         int32_t* ctx_dev, int32_t* step_dev, const int32_t* targets, int T, int ctx_upper, void* hidden,
                         void* logits, int ld_logits, void* workspace, size_t ws_bytes, float* lp, float* lse, int32_t* top1,
                         emu_stream_t s) {
    if (!m || !m->embed || !targets || !step_dev || !ctx_dev || T < 1) return -22;
    const ScoreSel sel{targets, T, lp, lse, top1};
    return llama_token_step(m, Bn, cur_ids, pos, slot, kstart, ctx_dev, step_dev, nullptr, 0, ctx_upper, hidden, logits, ld_logits,
                            workspace, ws_bytes, nullptr, nullptr, nullptr, &sel, nullptr, nullptr, 0, s);
}

int emu_lookup_select_bf16(const void* logits, int ld, int V, int T, int32_t* amax, int32_t* cur, int32_t* st, int32_t* pos0,
                           int32_t* slot0, int32_t* ctx_dev, int32_t* out_ids, int32_t* hist, int hist_cap, const int32_t* drafts,
                           int max_ngram, int max_new, int min_len, int eos_id, int stop_on_eos, emu_stream_t s) {
    const LookupArgs a{B(logits), ld, V, T, amax, cur, st, pos0, slot0, ctx_dev, out_ids, hist, hist_cap, drafts, max_ngram, max_new,
                       min_len, eos_id, stop_on_eos};
    int e = launch_lookup_argmax(a, S(s));
    if (e) return e;
    return launch_lookup_select(a, S(s));
}

int emu_lookup_sample_bf16(const void* logits, int ld, int V, int T, int32_t* amax, int32_t* cur, int32_t* st, int32_t* pos0,
                           int32_t* slot0, int32_t* ctx_dev, int32_t* out_ids, int32_t* hist, int hist_cap, const int32_t* drafts,
                           int max_ngram, int max_new, int min_len, int eos_id, int stop_on_eos, const emu_sample_params* params,
                           const float* uniforms, int uni_rows, emu_stream_t s) {
    const LookupArgs a{B(logits), ld, V, T, amax, cur, st, pos0, slot0, ctx_dev, out_ids, hist, hist_cap, drafts, max_ngram, max_new,
                       min_len, eos_id, stop_on_eos};
    if (!pos0 || !slot0 || !ctx_dev || !hist || max_ngram < 1 || hist_cap < 1) return -22;       // the select launch's, before the first
    int e = launch_lookup_sample(a, params, uniforms, uni_rows, S(s));
    if (e) return e;
    return launch_lookup_select(a, S(s));
}

// One step of the prompt-lookup loop: embed the T = 1 + k ids of `cur` (the last emitted id, then the draft) -> chunk forward -> final
// norm + logits on the T rows -> the rows' ids (params null: arg-maxes; else the sampler's selection, row i as output index step + i)
// -> accept / append / next draft / state advance (lookup.hip).  Capturable.
static int llama_lookup_step(emu_llama* m, int T, int32_t* cur, int32_t* amax, int32_t* st, int32_t* pos0, int32_t* slot0,
                             const int32_t* kstart, int32_t* ctx_dev, int32_t* out_ids, int32_t* hist, int hist_cap,
                             const int32_t* drafts, int max_ngram, int max_new, int min_len, int eos_id, int stop_on_eos, int ctx_upper,
                             void* hidden, void* logits, int ld_logits, void* workspace, size_t ws_bytes,
                             const emu_sample_params* params, const float* uniforms, int uni_rows, emu_stream_t s) {
    if (!m || !m->embed || !cur || !hidden || !logits) return -22;
    const emu_llama_cfg& c = m->cfg;
    const LookupArgs a{B(logits), ld_logits, c.vocab, T, amax, cur, st, pos0, slot0, ctx_dev, out_ids, hist, hist_cap, drafts, max_ngram,
                       max_new, min_len, eos_id, stop_on_eos};
    if (T < 2 || T > DECODE_CHUNK_MAX || !amax || !st || !pos0 || !slot0 || !ctx_dev || !out_ids || !hist || max_new < 1 || max_ngram < 1 ||
        hist_cap < 1)
        return -22;                                  // refused before anything is launched
    if (params && (ld_logits < c.vocab || !lookup_sample_ok(c.vocab, params, uniforms, uni_rows))) return -22;       // likewise
    if (m->prefix_len > 0) return fail(m->ctx, -22, "lookup step: a KV prefix serves emu_llama_forward with T > 1 only");
    TRY(m->ctx, launch_embed_gather(cur, m->embed, B(hidden), T, c.hidden, c.vocab, S(s)));
    TRY(m->ctx, emu_llama_forward_chunk(m, hidden, 1, T, pos0, slot0, kstart, ctx_dev, ctx_upper, workspace, ws_bytes, s));
    TRY(m->ctx, emu_llama_logits(m, hidden, c.hidden, T, logits, ld_logits, workspace, ws_bytes, s));
    if (params) TRY(m->ctx, launch_lookup_sample(a, params, uniforms, uni_rows, S(s)));
    else TRY(m->ctx, launch_lookup_argmax(a, S(s)));
    TRY(m->ctx, launch_lookup_select(a, S(s)));
    return 0;
}

int emu_llama_lookup_step(emu_llama* m, int T, int32_t* cur, int32_t* amax, int32_t* st, int32_t* pos0, int32_t* slot0,
                          const int32_t* kstart, int32_t* ctx_dev, int32_t* out_ids, int32_t* hist, int hist_cap, const int32_t* drafts,
                          int max_ngram, int max_new, int min_len, int eos_id, int stop_on_eos, int ctx_upper, void* hidden,
                          void* logits, int ld_logits, void* workspace, size_t ws_bytes, emu_stream_t s) {
    return llama_lookup_step(m, T, cur, amax, st, pos0, slot0, kstart, ctx_dev, out_ids, hist, hist_cap, drafts, max_ngram, max_new,
                             min_len, eos_id, stop_on_eos, ctx_upper, hidden, logits, ld_logits, workspace, ws_bytes, nullptr, nullptr, 0,
                             s);
}

int emu_llama_lookup_sample_step(emu_llama* m, int T, int32_t* cur, int32_t* amax, int32_t* st, int32_t* pos0, int32_t* slot0,
                                 const int32_t* kstart, int32_t* ctx_dev, int32_t* out_ids, int32_t* hist, int hist_cap,
                                 const int32_t* drafts, int max_ngram, int max_new, int min_len, int eos_id, int stop_on_eos,
                                 int ctx_upper, void* hidden, void* logits, int ld_logits, void* workspace, size_t ws_bytes,
                                 const emu_sample_params* params, const float* uniforms, int uni_rows, emu_stream_t s) {
    if (!params) return -22;
    return llama_lookup_step(m, T, cur, amax, st, pos0, slot0, kstart, ctx_dev, out_ids, hist, hist_cap, drafts, max_ngram, max_new,
                             min_len, eos_id, stop_on_eos, ctx_upper, hidden, logits, ld_logits, workspace, ws_bytes, params, uniforms,
                             uni_rows, s);
}

}  // extern "C"

// =============================================================================================== ViT engine
struct emu_vit {
    emu_ctx* ctx;
    emu_vit_cfg cfg;
    const bf16_t *wpatch = nullptr, *bpatch = nullptr, *cls = nullptr, *pos = nullptr;
    struct Block { const bf16_t *wqkv, *bqkv, *wproj, *bproj, *ln1w, *ln1b, *fc1w, *fc1b, *fc2w, *fc2b, *ln2w, *ln2b; };
    std::vector<Block> blocks;
    // optional fp8 (e4m3, one fp32 scale per output row) copies of the four matrices of every block: emu_vit_use_fp8 runs the
    // blocks' GEMMs W8A8 on the block-scaled MFMA, the activation rows quantised per row ahead of every GEMM
    struct Block8 { const uint8_t *wqkv = nullptr, *wproj = nullptr, *fc1w = nullptr, *fc2w = nullptr;
                    const float *sqkv = nullptr, *sproj = nullptr, *sfc1 = nullptr, *sfc2 = nullptr; };
    std::vector<Block8> blocks8;
    bool fp8 = false;
    bool fuse_vt = true;                             // emu_vit_set_fusion bit 0: V^T out of the qkv projection's epilogue (one image)
    bool fuse_norm = true;                           // bit 1: fc2's K-slice sum applies bias + LayerNorm + residual (post-norm blocks)
    // token-parallel encode of one image (emu_vit_set_token_parallel / emu_vit_forward_tp): this rank computes token rows
    // [tp_r0, tp_r1) of every block; the K rows and V^T key columns of the others arrive through the exchange regions (p2p.hip)
    int tp_rank = 0, tp_world = 0;                   // tp_world 0: not set
    bool tp_emulate = false;                         // timing tools: the exchanges are skipped (only this rank's rows are right)
    EmuVitX* xchg = nullptr;
    int tp_r0 = 0, tp_r1 = 0;                        // rows computed by the last emu_vit_forward_tp
    ~emu_vit() { emu_vitx_destroy(xchg); }
};

namespace {
constexpr int VIT_DP = 128;      // padded head dim
struct VitWs { bf16_t *patches, *pemb, *qkv, *vt, *attn, *tmp, *h1; float* splitk; size_t splitk_floats;
               uint8_t* x8; float* xs;           // fp8 mode: the current GEMM's activation rows as e4m3 bytes + per-row scales
               size_t total; };
VitWs vit_ws(const emu_vit* m, int Bn, void* base) {
    const emu_vit_cfg& c = m->cfg;
    const int g = c.image_size / c.patch_size, T = g * g, N = T + 1;
    const size_t M = (size_t)Bn * N;
    const size_t npad = (size_t)(N + 63) / 64 * 64;
    char* p = reinterpret_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
    VitWs w;
    w.patches = (bf16_t*)take((size_t)Bn * T * c.kpad * 2);
    w.pemb = (bf16_t*)take((size_t)Bn * T * c.width * 2);
    w.qkv = (bf16_t*)take(M * 3 * c.heads * VIT_DP * 2);
    w.vt = (bf16_t*)take((size_t)Bn * c.heads * VIT_DP * npad * 2);
    w.attn = (bf16_t*)take(M * c.heads * VIT_DP * 2);
    w.tmp = (bf16_t*)take(M * c.width * 2);
    w.h1 = (bf16_t*)take(M * (size_t)c.mlp_hidden * 2);
    w.splitk_floats = EMU_SPLITK_SCRATCH_FLOATS;          // K-slices of fc2 (63 tiles of 256x128) and of fc1's tail round
    w.splitk = (float*)take(w.splitk_floats * sizeof(float));
    const size_t kmax = std::max<size_t>(std::max<size_t>(c.width, (size_t)c.heads * VIT_DP), c.mlp_hidden);
    w.x8 = (uint8_t*)take(m->blocks8.empty() ? 0 : M * kmax);
    w.xs = (float*)take(m->blocks8.empty() ? 0 : M * sizeof(float));
    w.total = off;
    return w;
}
}  // namespace

extern "C" {

int emu_vit_create(emu_ctx* ctx, const emu_vit_cfg* cfg, emu_vit** out) {
    if (!ctx || !cfg || !out) return -22;
    if (cfg->head_width > VIT_DP || (cfg->width & 7) || (cfg->mlp_hidden & 7) || (cfg->kpad & 7) ||
        cfg->kpad < 3 * cfg->patch_size * cfg->patch_size || cfg->image_size % cfg->patch_size)
        return fail(ctx, -22, "emu_vit_create: unsupported shape");
    emu_vit* m = new emu_vit();
    m->ctx = ctx; m->cfg = *cfg;
    m->blocks.resize(cfg->layers);
    memset(m->blocks.data(), 0, sizeof(emu_vit::Block) * cfg->layers);
    *out = m;
    return 0;
}
void emu_vit_destroy(emu_vit* m) { delete m; }
int emu_vit_set_stem(emu_vit* m, const void* wpatch, const void* bpatch, const void* cls, const void* pos) {
    if (!m) return -22;
    m->wpatch = B(wpatch); m->bpatch = B(bpatch); m->cls = B(cls); m->pos = B(pos);
    return 0;
}
int emu_vit_set_block(emu_vit* m, int layer, const void* wqkv, const void* bqkv, const void* wproj, const void* bproj,
                      const void* ln1w, const void* ln1b, const void* fc1w, const void* fc1b, const void* fc2w,
                      const void* fc2b, const void* ln2w, const void* ln2b) {
    if (!m || layer < 0 || layer >= m->cfg.layers) return -22;
    m->blocks[layer] = {B(wqkv), B(bqkv), B(wproj), B(bproj), B(ln1w), B(ln1b), B(fc1w), B(fc1b), B(fc2w), B(fc2b), B(ln2w), B(ln2b)};
    return 0;
}
int emu_vit_set_block_fp8(emu_vit* m, int layer, const void* wqkv8, const float* sqkv, const void* wproj8, const float* sproj,
                          const void* fc1w8, const float* sfc1, const void* fc2w8, const float* sfc2) {
    if (!m || layer < 0 || layer >= m->cfg.layers) return -22;
    if (!wqkv8 || !sqkv || !wproj8 || !sproj || !fc1w8 || !sfc1 || !fc2w8 || !sfc2) return -22;
    const emu_vit_cfg& c = m->cfg;
    if ((c.width & 127) || (c.mlp_hidden & 127))
        return fail(m->ctx, -22, "emu_vit_set_block_fp8: width and mlp_hidden must be multiples of 128 (k tiles of the fp8 MFMA)");
    if (m->blocks8.size() != (size_t)c.layers) m->blocks8.assign(c.layers, emu_vit::Block8{});
    auto U = [](const void* p) { return reinterpret_cast<const uint8_t*>(p); };
    m->blocks8[layer] = {U(wqkv8), U(wproj8), U(fc1w8), U(fc2w8), sqkv, sproj, sfc1, sfc2};
    return 0;
}
int emu_vit_set_fusion(emu_vit* m, int mask) {
    if (!m) return -22;
    m->fuse_vt = (mask & 1) != 0;
    m->fuse_norm = (mask & 2) != 0;
    return 0;
}
int emu_vit_use_fp8(emu_vit* m, int enable) {
    if (!m) return -22;
    if (enable) {
        if (m->blocks8.size() != (size_t)m->cfg.layers) return fail(m->ctx, -22, "emu_vit_use_fp8: fp8 block weights not set");
        for (const auto& b : m->blocks8)
            if (!b.wqkv) return fail(m->ctx, -22, "emu_vit_use_fp8: fp8 block weights not set");
    }
    m->fp8 = enable != 0;
    return 0;
}
size_t emu_vit_workspace_bytes(const emu_vit* m, int Bn) { return m ? vit_ws(m, Bn, nullptr).total : 0; }

// token rows [rows[r], rows[r + 1]) of rank r (emu_amd/tp.py::token_rows): ceil(N / 8) groups of 8 rows, rank r starting at group
// ceil(r * groups / world) -- contiguous, balanced to one group, row 0 (CLS) on rank 0, a trailing rank may own none
static void vit_token_rows(int N, int world, int* rows) {
    const long U = (N + 7) / 8;
    for (int r = 0; r <= world; ++r) rows[r] = std::min<long>(8 * ((r * U + world - 1) / world), N);
}

// one image's rows [r0, r1) of the token-parallel chain; rows: the partition of every rank, xchg: the exchange (null: skipped)
struct VitTp { int r0, r1; const int* rows; EmuVitX* xchg; };

// blocks [l0, l1) in place on tokens x [B * N, C]; tp: only rows [tp->r0, tp->r1) of one image (x and the qkv / V^T buffers stay
// full size, own rows at their global offsets), every block's K rows and V^T keys exchanged between the qkv projection and attention
static int vit_blocks(emu_vit* m, bf16_t* x, int Bn, int l0, int l1, const VitWs& w, hipStream_t s, const VitTp* tp = nullptr) {
    emu_ctx* cx = m->ctx;
    const emu_vit_cfg& c = m->cfg;
    const int g = c.image_size / c.patch_size, T = g * g, N = T + 1, C = c.width, Hh = c.heads;
    const int QK = Hh * VIT_DP, F = c.mlp_hidden;
    const int npad = (N + 63) / 64 * 64;
    const float scale = 1.0f / sqrtf((float)c.head_width);
    const int r0 = tp ? tp->r0 : 0, M = tp ? tp->r1 - tp->r0 : Bn * N;   // rows this call computes
    x += (size_t)r0 * C;
    // one GEMM of a block: bf16, or (emu_vit_use_fp8) the activation rows quantised per row + the fp8 x fp8 GEMM
    // (quantised = true: the LayerNorm in front of this GEMM has left the rows in w.x8 / w.xs already: launch_layernorm_q8)
    auto lin = [&](const bf16_t* A, const bf16_t* W, const uint8_t* W8, const float* ws8, const bf16_t* bias, const bf16_t* res,
                   bf16_t* Cc, int N_, int K_, int ldres, int epi, bool quantised = false) -> int {
        if (!W8)
            return linear(A, W, bias, res, nullptr, Cc, M, N_, K_, K_, K_, ldres, N_, 0.f, epi, s, nullptr, w.splitk, w.splitk_floats);
        if (!quantised) {
            const int st = launch_quant_fp8_rows(A, K_, w.x8, K_, w.xs, M, K_, s);
            if (st) return st;
        }
        GemmArgs ga{reinterpret_cast<const bf16_t*>(w.x8), reinterpret_cast<const bf16_t*>(W8), bias, res, Cc, M, N_, K_, K_, K_, ldres, N_,
                    epi, ConvGeom{0, 0, 0, 0, 0, 0}, nullptr, 0, 0};
        ga.a_scale = w.xs; ga.w_scale = ws8;
        ga.partial = w.splitk; ga.partial_floats = w.splitk_floats;
        return launch_gemm_fp8(ga, s);
    };
    // V^T out of the qkv epilogue (one image, bf16) writes keys [0, N) and the few pad keys of the last 8-key group; the rest of the
    // pad columns [N, npad) of the V^T buffer is nobody's: zeroed once per call (the attention kernel multiplies them by masked
    // probabilities, and a stale NaN pattern times zero is NaN)
    if ((m->fuse_vt || tp) && Bn == 1 && !m->fp8 && npad != N && l1 > l0 &&
        hipMemsetAsync(w.vt, 0, (size_t)Hh * VIT_DP * npad * 2, s) != hipSuccess)
        return fail(cx, -5, "emu_vit_forward: hipMemsetAsync");
    const bool q8 = m->fp8 && C <= 2048;                 // LayerNorm rows leave as fp8 operands (launch_layernorm_q8)
    bool x8_valid = false;                               // post-norm: w.x8 / w.xs hold the quantised rows of x
    for (int l = l0; l < l1; ++l) {
        const emu_vit::Block& Bk = m->blocks[l];
        if (!Bk.wqkv) return fail(cx, -22, "emu_vit_forward: block weights not set");
        const emu_vit::Block8 B8 = m->fp8 ? m->blocks8[l] : emu_vit::Block8{};
        const bf16_t* ain = x;                           // attention input
        if (M == 0) {                                    // a rank without rows still takes part in every exchange
            if (tp->xchg) TRY(cx, emu_vitx_exchange(tp->xchg, tp->rows, w.qkv + QK, 3 * QK, QK, w.vt, npad, s));
            continue;
        }
        if (c.prenorm) {
            if (q8) TRY(cx, launch_layernorm_q8(x, Bk.ln1w, Bk.ln1b, nullptr, nullptr, w.x8, w.xs, M, C, c.ln_eps, s));
            else TRY(cx, launch_layernorm(x, Bk.ln1w, Bk.ln1b, nullptr, w.tmp, M, C, c.ln_eps, s));
            ain = w.tmp;
        }
        // one image, bf16: the V heads leave the qkv projection key-contiguous (GemmArgs::vt_*, round 3's UNet epilogue; the
        // transposed staging takes a single batch element's ragged last tile since round 4) -- no transpose launch
        const bool fvt = (m->fuse_vt || tp) && Bn == 1 && !B8.wqkv;
        if (fvt) {
            // token-parallel: own rows land at row r0 of the qkv buffer and at key r0 of V^T (r0 is a multiple of 8: 16-byte aligned)
            GemmArgs gq{ain, Bk.wqkv, Bk.bqkv, nullptr, w.qkv + (size_t)r0 * 3 * QK, M, 3 * QK, C, C, C, 0, 3 * QK, EPI_NONE, ConvGeom{0, 0, 0, 0, 0, 0}, nullptr, 0, 0};
            gq.partial = w.splitk; gq.partial_floats = w.splitk_floats;
            gq.vt_out = w.vt + r0; gq.vt_col0 = 2 * QK; gq.vt_s = M; gq.vt_spad = npad;
            TRY(cx, launch_gemm(gq, s));
        } else {
            TRY(cx, lin(ain, Bk.wqkv, B8.wqkv, B8.sqkv, Bk.bqkv, nullptr, w.qkv, 3 * QK, C, 0, EPI_NONE, q8 && (c.prenorm || x8_valid)));
            TransposeVArgs tv{w.qkv + 2 * QK, (long)N * 3 * QK, (long)VIT_DP, (long)3 * QK, w.vt, Bn, Hh, N, VIT_DP, npad};
            TRY(cx, launch_transpose_v(tv, s));
        }
        if (tp && tp->xchg) TRY(cx, emu_vitx_exchange(tp->xchg, tp->rows, w.qkv + QK, 3 * QK, QK, w.vt, npad, s));
        FlashArgs f{w.qkv + (size_t)r0 * 3 * QK, (long)N * 3 * QK, (long)VIT_DP, (long)3 * QK,
                    w.qkv + QK, (long)N * 3 * QK, (long)VIT_DP, (long)3 * QK,
                    w.vt, w.attn, (long)N * QK, (long)VIT_DP, (long)QK, nullptr,
                    Bn, Hh, tp ? M : N, N, npad, VIT_DP, 0, scale};
        TRY(cx, launch_flash_attn(f, s));
        if (c.prenorm) {
            // x = x + proj(attn);  x = x + fc2(gelu(fc1(LN2(x))))
            TRY(cx, lin(w.attn, Bk.wproj, B8.wproj, B8.sproj, Bk.bproj, x, x, C, QK, C, EPI_RESID));
            if (q8) TRY(cx, launch_layernorm_q8(x, Bk.ln2w, Bk.ln2b, nullptr, nullptr, w.x8, w.xs, M, C, c.ln_eps, s));
            else TRY(cx, launch_layernorm(x, Bk.ln2w, Bk.ln2b, nullptr, w.tmp, M, C, c.ln_eps, s));
            TRY(cx, lin(w.tmp, Bk.fc1w, B8.fc1w, B8.sfc1, Bk.fc1b, nullptr, w.h1, F, C, 0, EPI_GELU, q8));
            TRY(cx, lin(w.h1, Bk.fc2w, B8.fc2w, B8.sfc2, Bk.fc2b, x, x, C, F, C, EPI_RESID));
        } else {
            TRY(cx, lin(w.attn, Bk.wproj, B8.wproj, B8.sproj, Bk.bproj, nullptr, w.tmp, C, QK, 0, EPI_NONE));
            if (q8) TRY(cx, launch_layernorm_q8(w.tmp, Bk.ln1w, Bk.ln1b, x, x, w.x8, w.xs, M, C, c.ln_eps, s));
            else TRY(cx, launch_layernorm(w.tmp, Bk.ln1w, Bk.ln1b, x, x, M, C, c.ln_eps, s));
            TRY(cx, lin(x, Bk.fc1w, B8.fc1w, B8.sfc1, Bk.fc1b, nullptr, w.h1, F, C, 0, EPI_GELU, q8));
            // bf16: fc2 is a K-sliced GEMM (28 big tiles, K = 15360): its slice sum applies bias, LayerNorm and the residual add
            // row-wise in the same launch (GemmArgs::norm_*; -95 = this shape is not sliced that way: the launches apart)
            int st2 = -95;
            if (m->fuse_norm && !B8.fc2w) {
                GemmArgs gf{w.h1, Bk.fc2w, Bk.fc2b, nullptr, nullptr, M, C, F, F, F, 0, C, EPI_NONE, ConvGeom{0, 0, 0, 0, 0, 0}, nullptr, 0, 0};
                gf.partial = w.splitk; gf.partial_floats = w.splitk_floats;
                gf.norm_w = Bk.ln2w; gf.norm_b = Bk.ln2b; gf.norm_res = x; gf.norm_ldres = C; gf.norm_out = x; gf.norm_ld = C; gf.norm_eps = c.ln_eps;
                st2 = launch_gemm(gf, s);
                if (st2 != 0 && st2 != -95) return fail(cx, st2, "emu_vit_forward: fc2 with the LayerNorm slice sum");
            }
            if (st2 == -95) {
                TRY(cx, lin(w.h1, Bk.fc2w, B8.fc2w, B8.sfc2, Bk.fc2b, nullptr, w.tmp, C, F, 0, EPI_NONE));
                if (q8) TRY(cx, launch_layernorm_q8(w.tmp, Bk.ln2w, Bk.ln2b, x, x, w.x8, w.xs, M, C, c.ln_eps, s));   // the next block's qkv rows
                else TRY(cx, launch_layernorm(w.tmp, Bk.ln2w, Bk.ln2b, x, x, M, C, c.ln_eps, s));
            }
            x8_valid = q8;
        }
    }
    return 0;
}

int emu_vit_forward(emu_vit* m, const void* image, int image_is_f32, int Bn, void* out_tokens, void* workspace,
                    size_t ws_bytes, emu_stream_t s_) {
    if (!m || !image || !out_tokens || !m->wpatch) return -22;
    emu_ctx* cx = m->ctx;
    const emu_vit_cfg& c = m->cfg;
    const VitWs w = vit_ws(m, Bn, workspace);
    if (w.total > ws_bytes) return fail(cx, -12, "emu_vit_forward: workspace too small");
    hipStream_t s = S(s_);
    const int g = c.image_size / c.patch_size, T = g * g, C = c.width;
    bf16_t* x = B(out_tokens);
    TRY(cx, launch_patchify(image, image_is_f32, w.patches, Bn, 3, c.image_size, c.patch_size, c.kpad, s));
    TRY(cx, linear(w.patches, m->wpatch, m->bpatch, nullptr, nullptr, w.pemb, Bn * T, C, c.kpad, c.kpad, c.kpad, 0, C, 0.f, EPI_NONE, s));
    TRY(cx, launch_vit_assemble(w.pemb, m->cls, m->pos, x, Bn, T, C, s));
    return vit_blocks(m, x, Bn, 0, c.layers, w, s);
}

int emu_vit_set_token_parallel(emu_vit* m, int rank, int world, int emulate) {
    if (!m || world < 1 || world > EMU_P2P_MAX_RANKS || rank < 0 || rank >= world) return -22;
    if (m->xchg && (world != m->tp_world || rank != m->tp_rank)) { emu_vitx_destroy(m->xchg); m->xchg = nullptr; }
    m->tp_rank = rank; m->tp_world = world; m->tp_emulate = emulate != 0;
    return 0;
}
int emu_vit_tp_create(emu_vit* m, void* handle64_out) {
    if (!m || !handle64_out || m->tp_world < 2) return -22;
    if (m->xchg) return fail(m->ctx, -17, "emu_vit_tp_create: already created");
    hipError_t e = hipSetDevice(m->ctx->device);
    if (e != hipSuccess) return fail(m->ctx, (int)e, "hipSetDevice");
    const emu_vit_cfg& c = m->cfg;
    const int g = c.image_size / c.patch_size, N = g * g + 1, QK = c.heads * VIT_DP;
    m->xchg = emu_vitx_create(m->tp_rank, m->tp_world, (size_t)N * std::max(QK, c.width), QK, (N + 63) / 64 * 64, handle64_out);
    return m->xchg ? 0 : fail(m->ctx, -12, "emu_vit_tp_create: exchange region allocation / IPC export failed");
}
int emu_vit_tp_open(emu_vit* m, const void* handles, int timeout_ms, int fenced) {
    if (!m || !m->xchg) return -22;
    hipError_t e = hipSetDevice(m->ctx->device);
    if (e != hipSuccess) return fail(m->ctx, (int)e, "hipSetDevice");
    const int st = emu_vitx_open(m->xchg, handles, timeout_ms, fenced);
    return st == 0 ? 0 : fail(m->ctx, st, "emu_vit_tp_open: hipIpcOpenMemHandle");
}
int emu_vit_tp_rows(const emu_vit* m, int* r0, int* r1) {
    if (!m || !r0 || !r1) return -22;
    *r0 = m->tp_r0; *r1 = m->tp_r1;
    return 0;
}

int emu_vit_forward_tp(emu_vit* m, const void* image, int image_is_f32, void* out_tokens, void* workspace, size_t ws_bytes,
                       emu_stream_t s_) {
    if (!m || !image || !out_tokens || !m->wpatch) return -22;
    emu_ctx* cx = m->ctx;
    if (m->tp_world < 1) return fail(cx, -22, "emu_vit_forward_tp: emu_vit_set_token_parallel first");
    if (m->fp8) return fail(cx, -22, "emu_vit_forward_tp: the fp8 blocks have no token-parallel form");
    if (m->tp_world > 1 && !m->tp_emulate && !m->xchg) return fail(cx, -107, "emu_vit_forward_tp: exchange region not opened");
    const emu_vit_cfg& c = m->cfg;
    const VitWs w = vit_ws(m, 1, workspace);
    if (w.total > ws_bytes) return fail(cx, -12, "emu_vit_forward_tp: workspace too small");
    hipStream_t s = S(s_);
    const int g = c.image_size / c.patch_size, T = g * g, N = T + 1, C = c.width;
    int rows[EMU_P2P_MAX_RANKS + 1];
    vit_token_rows(N, m->tp_world, rows);
    const int r0 = rows[m->tp_rank], r1 = rows[m->tp_rank + 1];
    EmuVitX* xg = m->tp_world > 1 && !m->tp_emulate ? m->xchg : nullptr;
    bf16_t* x = B(out_tokens);
    // stem: own patches only (token t > 0 is patch t - 1; the CLS row belongs to rank 0)
    if (r1 > r0) {
        TRY(cx, launch_patchify(image, image_is_f32, w.patches, 1, 3, c.image_size, c.patch_size, c.kpad, s));
        const int p0 = std::max(r0, 1) - 1, p1 = r1 - 1;
        if (p1 > p0)
            TRY(cx, linear(w.patches + (size_t)p0 * c.kpad, m->wpatch, m->bpatch, nullptr, nullptr, w.pemb + (size_t)p0 * C, p1 - p0, C, c.kpad,
                           c.kpad, c.kpad, 0, C, 0.f, EPI_NONE, s));
        TRY(cx, launch_vit_assemble_rows(w.pemb, m->cls, m->pos, x, r0, r1, C, s));
    }
    const VitTp tp{r0, r1, rows, xg};
    m->tp_r0 = r0; m->tp_r1 = r1;
    TRY(cx, vit_blocks(m, x, 1, 0, c.layers, w, s, &tp));
    // every rank ends with the same bytes: the final token rows are gathered once
    if (xg) TRY(cx, emu_vitx_exchange(xg, rows, x, C, C, nullptr, 0, s));
    return 0;
}

int emu_vit_blocks(emu_vit* m, void* tokens, int Bn, int l0, int l1, void* workspace, size_t ws_bytes, emu_stream_t s_) {
    if (!m || !tokens || l0 < 0 || l1 > m->cfg.layers || l1 < l0) return -22;
    const VitWs w = vit_ws(m, Bn, workspace);
    if (w.total > ws_bytes) return fail(m->ctx, -12, "emu_vit_blocks: workspace too small");
    return vit_blocks(m, B(tokens), Bn, l0, l1, w, S(s_));
}

}  // extern "C"
