// L2 warming across a kernel boundary of the one-row decode step (DESIGN 4a').
//
// Every address the NEXT launch on the stream will read is known on the host (weights do not depend on activations), and the only
// storage on the XCD side of the fabric that survives a kernel boundary is the L2 (4 MiB per XCD).  So a few workgroups of a launch
// -- its last ones, or extra ones behind the working grid -- request the first bytes the next launch's workgroups will read:
// one default-policy dword load per 128-byte line, never waited for, result discarded.  Workgroups are dealt to the XCDs round-robin
// by their linear id (observed, not guaranteed: MI355X_MICROARCH.md), so a line that successor workgroup j will read is requested
// from a workgroup of the same id % xcds, and lands in the L2 that j's XCD looks in.  This is for speed only: whatever the touches
// hit or miss, nothing is read back, nothing is waited for, and results do not depend on them.
//
// The plan is a POD in the kernel-argument segment.  warm_line() is the ONE place that maps (toucher workgroup, thread, trip) to a
// line; the device loop (warm_touch) and the host enumerator (emu_l2_warm_enumerate, tests/test_l2_warm_plan.py) both call it.
//
// Successor geometry: workgroup j (linear id, x + gx * (y + gy * z) for a 3-D grid) reads `rows` rows of `row_bytes` stride from
//     base + j * block_bytes                                   (gx == 0: a weight stream, block j = rows [j * R, j * R + R))
//     base + (j % gx) * block_bytes + (j / gx) * group_bytes   (gx > 0: decode attention, j = split + gx * head: 128 cache slots)
// and of every row the first head_bytes are warmed (head_bytes == the row's used bytes: whole blocks; less: the first trip).
// twin != 0: a second array of the same geometry at base + twin (the V cache behind the K cache).
// Invariants (checked on the CPU): every line lies wholly inside [base, base + limit) (+ twin); no line is requested twice; at most
// `nsucc * rows * ceil(head_bytes / 128)` (x 2 with a twin) lines, which make_warm_plan keeps within the budget; toucher and reader
// (the workgroup whose block the line STARTS in) have the same id % xcds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EMU_WARM_HD __host__ __device__ inline
#else
#define EMU_WARM_HD inline
#endif

struct WarmPlan {
    const char* base = nullptr;     // the successor's first byte (128-byte aligned); ntouch == 0: no warming
    int64_t twin = 0;               // 0, or the byte distance to a second array of the same geometry
    uint64_t limit = 0;             // bytes of the successor array: every line ends at or before base + limit
    uint64_t group_bytes = 0;       // gx > 0: bytes between the blocks of consecutive groups (heads)
    uint32_t block_bytes = 0;       // bytes per successor workgroup block = rows per workgroup x row_bytes
    uint32_t row_bytes = 0;         // row stride
    uint32_t head_bytes = 0;        // leading bytes of every row that are warmed
    uint32_t nsucc = 0;             // successor workgroups covered: linear ids [0, nsucc)
    uint32_t gx = 0;                // 0: flat; else blocks per group
    uint32_t first = 0, ntouch = 0; // toucher workgroups: linear ids [first, first + ntouch) of the predecessor's grid
    uint32_t lanes = 256;           // threads of a toucher workgroup
    uint32_t xcds = 8;
};

// ids in [0, e) that are congruent to c modulo x
EMU_WARM_HD uint32_t warm_count(uint32_t e, uint32_t c, uint32_t x) { return (e + x - 1 - c) / x; }

// The work of a class (the touchers and the successor blocks of one id % xcds) is cut into UNITS: one row of one block and
// `lanes` consecutive lines of it, so that everything but the line within the unit is uniform over the workgroup (scalar
// registers on the device: the loop costs the kernels that carry it two vector registers).  The class's touchers take the units
// round-robin, one per trip.
struct WarmUnit {
    int64_t start;                  // byte offset from base of the unit's first candidate line (128-byte aligned); < 0: no unit
    uint32_t span;                  // thread t requests the line at start + 128 t where 128 t < span
};
// units of one array per class c, and chunks of `lanes` lines per row
EMU_WARM_HD uint32_t warm_chunks(const WarmPlan& p) { return (((p.head_bytes + 127u) >> 7) + p.lanes - 1) / p.lanes; }
EMU_WARM_HD uint32_t warm_class_units(const WarmPlan& p, uint32_t c) {
    return warm_count(p.nsucc, c, p.xcds) * (p.block_bytes / p.row_bytes) * warm_chunks(p) * (p.twin ? 2u : 1u);
}
// touchers of wg's class, and wg's rank among them
EMU_WARM_HD uint32_t warm_class_touchers(const WarmPlan& p, uint32_t c) {
    return warm_count(p.first + p.ntouch, c, p.xcds) - warm_count(p.first, c, p.xcds);
}

// trips of toucher workgroup wg (0: wg is no toucher)
EMU_WARM_HD uint32_t warm_trips(const WarmPlan& p, uint32_t wg) {
    if (!p.ntouch || wg < p.first || wg - p.first >= p.ntouch) return 0;
    const uint32_t c = wg % p.xcds, nc = warm_class_touchers(p, c);
    return (warm_class_units(p, c) + nc - 1) / nc;
}

// the unit toucher workgroup wg works on in trip i (uniform over the workgroup)
EMU_WARM_HD WarmUnit warm_unit(const WarmPlan& p, uint32_t wg, uint32_t i) {
    WarmUnit none{-1, 0};
    if (!p.ntouch || wg < p.first || wg - p.first >= p.ntouch) return none;
    const uint32_t x = p.xcds, c = wg % x;
    const uint32_t u = warm_count(wg, c, x) - warm_count(p.first, c, x);              // rank among the class's touchers
    const uint32_t R = p.block_bytes / p.row_bytes, CH = warm_chunks(p);
    const uint32_t per = R * CH, one = warm_count(p.nsucc, c, x) * per;              // units of one array
    uint32_t v = i * warm_class_touchers(p, c) + u;
    if (v >= one * (p.twin ? 2u : 1u)) return none;
    const bool second = v >= one;
    if (second) v -= one;
    const uint32_t m = v / per, q = v - m * per, r = q / CH, ch = q - r * CH;
    const uint32_t j = c + x * m;                                                    // the reader's linear workgroup id
    uint64_t blk;
    if (p.gx) {
        const uint32_t jx = j % p.gx, jg = j / p.gx;
        if ((uint64_t)(jx + 1) * p.block_bytes > p.group_bytes) return none;         // a block that leaves its group: skipped whole
        blk = (uint64_t)jx * p.block_bytes + (uint64_t)jg * p.group_bytes;
    } else {
        blk = (uint64_t)j * p.block_bytes;
    }
    const uint64_t row = blk + (uint64_t)r * p.row_bytes;
    // lines that START inside the row's head [row, row + head_bytes) and end inside the array, from the ch-th chunk on
    const uint64_t s = ((row + 127u) & ~(uint64_t)127u) + (uint64_t)ch * p.lanes * 128u;
    uint64_t end = row + p.head_bytes;
    if (p.limit < 127u) return none;
    if (end > p.limit - 127u) end = p.limit - 127u;
    if (s >= end) return none;
    const uint64_t span = end - s;
    return WarmUnit{(int64_t)s + (second ? p.twin : 0), (uint32_t)(span < (uint64_t)p.lanes * 128u ? span : (uint64_t)p.lanes * 128u)};
}

// Byte offset from p.base of the 128-byte line that thread tid of toucher workgroup wg requests in trip i, or -1 for none.
EMU_WARM_HD int64_t warm_line(const WarmPlan& p, uint32_t wg, uint32_t tid, uint32_t i) {
    const WarmUnit un = warm_unit(p, wg, i);
    if (un.start < 0 || tid >= p.lanes || tid * 128u >= un.span) return -1;
    return un.start + (int64_t)tid * 128;
}

#if defined(__HIPCC__)
// The device loop: this workgroup's share of the plan (nothing for a workgroup that is no toucher: one uniform compare).  The same
// warm_unit as warm_line; the lane's part is the 32-bit offset 128 tid against the unit's scalar base.  Returns the loads'
// destination register; the caller keeps it alive to the end of the kernel -- asm volatile("" :: "v"(d)) -- because a dword may
// land at any time before the wave ends (gemm_tile.h::prefetch_lines has the story of a register that was reused).
__device__ __forceinline__ uint32_t warm_touch(const WarmPlan& p, uint32_t wg, uint32_t tid) {
    uint32_t d = 0;
    if (p.ntouch != 0 && wg >= p.first) {
        const uint32_t n = warm_trips(p, wg);
        const uint32_t lane = tid * 128u;
        for (uint32_t i = 0; i < n; ++i) {
            const WarmUnit un = warm_unit(p, wg, i);
            if (un.start >= 0 && lane < un.span)
                asm volatile("global_load_dword %0, %1, %2" : "+v"(d) : "v"(lane), "s"(p.base + un.start) : "memory");
        }
    }
    return d;
}
#endif

// ---- host side: the successor as its launch reads it, and the plan for one boundary
struct WarmSucc {
    const void* base = nullptr;
    int64_t twin = 0;
    uint32_t rows = 0;              // rows per successor workgroup
    uint32_t row_bytes = 0;         // row stride
    uint32_t used_bytes = 0;        // bytes of a row the successor reads (K * 2)
    uint64_t nrows = 0;             // rows of the array (flat), or rows of one group (gx > 0)
    uint32_t gx = 0, groups = 1;    // gx > 0: blocks per group the successor's grid has, and groups
};
enum WarmShape { WARM_WHOLE_BLOCKS = 0, WARM_FIRST_TRIP = 1 };
constexpr uint32_t WARM_TRIP_BYTES = 4096;       // 256 threads x 16 bytes: what a stream workgroup requests of a row first
constexpr uint32_t WARM_TRIPS = 2;               // units a toucher workgroup takes where the predecessor has enough workgroups

// pred_wgs: the predecessor's working grid (linear).  extra = false: its last workgroups touch; extra = true: plan.ntouch workgroups
// BEHIND the working grid do (the caller enlarges its grid by plan.ntouch).  Empty (ntouch == 0) where the successor is smaller than
// one block, a predecessor whose own workgroups touch has fewer than xcds of them, the base is not line-aligned or the budget buys no block.
inline WarmPlan make_warm_plan(const WarmSucc& s, uint32_t pred_wgs, bool extra, uint32_t lanes, uint64_t budget_bytes, int shape) {
    WarmPlan p;
    const uint32_t x = p.xcds;
    if (!s.base || (reinterpret_cast<uintptr_t>(s.base) & 127u) || (s.twin & 127) || !s.rows || !s.row_bytes || !s.used_bytes ||
        s.used_bytes > s.row_bytes || s.nrows < s.rows || (!extra && pred_wgs < x) || !lanes)
        return p;
    const uint64_t block = (uint64_t)s.rows * s.row_bytes;
    if (block > 0xffffffffull) return p;
    p.base = reinterpret_cast<const char*>(s.base);
    p.twin = s.twin;
    p.block_bytes = (uint32_t)block;
    p.row_bytes = s.row_bytes;
    p.head_bytes = shape == WARM_FIRST_TRIP && s.used_bytes > WARM_TRIP_BYTES ? WARM_TRIP_BYTES : s.used_bytes;
    p.lanes = lanes;
    uint64_t blocks;
    if (s.gx) {
        p.gx = s.gx;
        p.group_bytes = s.nrows * s.row_bytes;
        p.limit = p.group_bytes * s.groups;
        blocks = (uint64_t)s.gx * s.groups;
    } else {
        p.limit = (s.nrows - 1) * s.row_bytes + s.used_bytes;
        blocks = (s.nrows + s.rows - 1) / s.rows;
    }
    const uint64_t lines_per_block = (uint64_t)s.rows * ((p.head_bytes + 127u) >> 7) * (s.twin ? 2 : 1);
    uint64_t n = (budget_bytes >> 7) / lines_per_block;
    if (n > blocks) n = blocks;
    if (n >= x) n -= n % x;                          // the same number of blocks for every class
    if (n == 0 || n * lines_per_block > 0x3fffffffull) return WarmPlan{};
    p.nsucc = (uint32_t)n;
    // whole blocks of rows that follow each other without a gap are one span: its lines fill the threads of a unit better
    if (p.head_bytes == s.row_bytes && s.rows > 1) p.row_bytes = p.head_bytes = p.block_bytes;
    const uint64_t units = n * (p.block_bytes / p.row_bytes) * warm_chunks(p) * (s.twin ? 2 : 1);
    uint64_t want = (units + WARM_TRIPS - 1) / WARM_TRIPS;
    want = (want + x - 1) / x * x;                   // whole rounds of the XCDs
    if (extra) {
        p.first = pred_wgs;
        p.ntouch = (uint32_t)want;
    } else {
        p.ntouch = (uint32_t)(want < pred_wgs ? want : pred_wgs);
        p.first = pred_wgs - p.ntouch;
    }
    return p;
}
