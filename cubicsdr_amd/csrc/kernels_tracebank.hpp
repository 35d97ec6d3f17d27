// kernels_tracebank.hpp -- the trace bank (gfx950): the spectrum, hold and scope lines of any number of items as tiles of one RGBA8 atlas.
//
//   spectrum trace and its peak-hold trace      src/panel/SpectrumPanel.cpp:117-160           trace_lines (CSDR_TRACE_SPECTRUM)
//   scope trace, one or two channels, axes      src/panel/ScopePanel.cpp:30-67, :97-105       trace_lines (CSDR_TRACE_SCOPE_Y, _2Y; the empty tiles too)
//   scope points, additive                      src/panel/ScopePanel.cpp:69-82, :106-108      trace_xy    (CSDR_TRACE_SCOPE_XY)
//
// The picture is the library's own definition (include/csdr_hip.h, "Trace bank"); its arithmetic is stated once in trace_host.hpp and called from
// here.  ONE launch of each kernel draws every item of its kind: a record per tile, uploaded with the call, says where the tile's points lie.
// No atomics: a column's lit interval is a min / max reduction over the column's own vertices and its two neighbouring segments, and an XY pixel
// row is owned by one work-item.
// Home unit: csdr_tracebank.hip.
#pragma once
#include "common.hpp"
#include "kernels_waterfall.hpp"
#include "trace_host.hpp"

#if defined(CSDR_TU_TRACEBANK)
#define CSDR_KERNEL_TRACE CSDR_KERNEL
#else
#define CSDR_KERNEL_TRACE CSDR_KERNEL_ELSEWHERE
#endif

namespace csdr {

constexpr int kTrThreads = 256;
constexpr int kTrCols = 64;                  // columns of a tile to a workgroup of trace_lines: 256 bytes of every picture row
constexpr int kTrRows = kTrThreads / (kTrCols / 4);      // picture rows a workgroup stores at a time: 16 work-items of 4 pixels to a row
constexpr int kTrXyLds = 32 * 1024;          // trace_xy: hit counters of a workgroup's rows, one byte per pixel

struct TraceTile {
    const float *pts, *hold;   // device memory: the caller's, or the staged copy of host points
    int32_t n, stride;         // as the item's n; floats from one vertex to the next (1 + layout)
    int32_t kind;              // CSDR_TRACE_*; -1: an empty tile -- all-zero bytes
    int32_t tile;              // its place in the atlas: tile row tile / atlas_cols, tile column tile % atlas_cols
};
static_assert(sizeof(TraceTile) == 32, "TraceTile layout");

struct TraceColors { uint32_t bg, line, hold, major, minor; };      // RGBA8 as the picture holds it (R in the low byte); alpha: the background's only

struct TraceArgs {
    const TraceTile *tiles;
    uint32_t *out;             // [tile rows * height][atlas_cols * width] pixels, dense
    int width, height, atlas_cols;
    int col_blocks;            // trace_lines: workgroups along a tile row
    int rows_per;              // picture rows of a tile to a workgroup
    int wp;                    // trace_xy: bytes of a counter row, width rounded up to 4
    TraceColors col;
};

__device__ __forceinline__ int64_t trace_pixel(const TraceArgs &a, int tile, int row, int px) {
    return ((int64_t)(tile / a.atlas_cols) * a.height + row) * ((int64_t)a.atlas_cols * a.width) + (int64_t)(tile % a.atlas_cols) * a.width + px;
}
// (a + b + 1) >> 1 in each of the three colour bytes, the alpha of `under` kept
__device__ __forceinline__ uint32_t trace_average(uint32_t under, uint32_t over) {
    const uint32_t a = under & 0x00ffffffu, b = over & 0x00ffffffu;
    return ((a | b) - (((a ^ b) >> 1) & 0x007f7f7fu)) | (under & 0xff000000u);
}

// grid (line tiles * col_blocks, groups of rows_per rows).  Pass 1: the lit intervals of the workgroup's kTrCols columns into LDS, [which][lo | hi]
// [column].  A column's vertices are walked by G neighbouring lanes -- G the power of two from 4 to 64 that covers the vertices per column, so the
// lanes of a group read consecutive floats and a workgroup's columns one contiguous run -- and reduced by lane exchange; the first lane of the group
// adds the two neighbouring segments.  One barrier.  Pass 2: every work-item keeps the intervals of its 4 columns and walks down the rows, a
// 16-byte store each.  A workgroup of a later row group repeats pass 1: at most n / W + 4 vertices per column against rows_per * 16 bytes stored.
CSDR_KERNEL_TRACE __launch_bounds__(kTrThreads) void trace_lines(TraceArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *env = reinterpret_cast<int *>(smem);            // [2][2][kTrCols]
    const int tid = (int)threadIdx.x;
    const TraceTile tl = a.tiles[blockIdx.x / (unsigned)a.col_blocks];
    const int c0 = (int)(blockIdx.x % (unsigned)a.col_blocks) * kTrCols, nc = min(kTrCols, a.width - c0);
    const int py0 = (int)blockIdx.y * a.rows_per, py1 = min(a.height, py0 + a.rows_per);
    if (tl.kind >= 0) {
        for (int which = 0; which < 2; ++which) {
            const TracePoly pl = trace_poly(tl.pts, tl.hold, tl.n, tl.stride, tl.kind, a.height, which);
            int *lo_s = env + 2 * which * kTrCols, *hi_s = lo_s + kTrCols;
            if (pl.n == 0) {
                if (tid < kTrCols) { lo_s[tid] = INT_MAX; hi_s[tid] = -1; }
                continue;
            }
            int G = 4;
            while (G < kTrCols && (int64_t)G * a.width < pl.n) G <<= 1;
            const int per = kTrThreads / G, sub = tid & (G - 1);
            for (int cbase = 0; cbase < kTrCols; cbase += per) {
                const int cl = cbase + tid / G, c = c0 + cl;
                int lo = INT_MAX, hi = -1;
                int64_t v0 = 0, v1 = 0;
                if (cl < nc) {
                    v0 = trace_first_vertex(c, pl.n, a.width); v1 = trace_first_vertex((int64_t)c + 1, pl.n, a.width);
                    for (int64_t i = v0 + sub; i < v1; i += G) { const int r = trace_row(pl, i); lo = min(lo, r); hi = max(hi, r); }
                }
                for (int o = 1; o < G; o <<= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
                if (sub == 0) {
                    if (cl < nc) trace_neighbours(pl, a.width, c, v0, v1, lo, hi);
                    lo_s[cl] = lo; hi_s[cl] = hi;
                }
            }
        }
    }
    __syncthreads();
    const int lane = tid & (kTrCols / 4 - 1), px0 = c0 + 4 * lane, cnt = min(4, a.width - px0);
    if (cnt <= 0) return;
    int lo0[4], hi0[4], lo1[4], hi1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool lit = tl.kind >= 0 && k < cnt;
        lo0[k] = lit ? env[4 * lane + k] : INT_MAX; hi0[k] = lit ? env[kTrCols + 4 * lane + k] : -1;
        lo1[k] = lit ? env[2 * kTrCols + 4 * lane + k] : INT_MAX; hi1[k] = lit ? env[3 * kTrCols + 4 * lane + k] : -1;
    }
    const TraceAxes ax = trace_axes(tl.kind, a.height);
    const bool blend = trace_hold_blends(tl.kind);
    const uint32_t alpha = a.col.bg & 0xff000000u, line = (a.col.line & 0x00ffffffu) | alpha;
    for (int r = py0 + tid / (kTrCols / 4); r < py1; r += kTrRows) {
        uint32_t px[4];
        const uint32_t under = tl.kind < 0 ? 0u : (r == ax.major ? (a.col.major & 0x00ffffffu) | alpha : (r == ax.minor0 || r == ax.minor1 ? (a.col.minor & 0x00ffffffu) | alpha : a.col.bg));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t v = r >= lo0[k] && r <= hi0[k] ? line : under;
            if (r >= lo1[k] && r <= hi1[k]) v = blend ? trace_average(v, a.col.hold) : line;
            px[k] = v;
        }
        wf_store4(a.out, trace_pixel(a, tl.tile, r, px0), cnt, px[0], px[1], px[2], px[3]);
    }
}

// grid (XY tiles, groups of rows_per rows), rows_per <= kTrThreads and rows_per * wp <= kTrXyLds.  The counters of the workgroup's rows are cleared
// in LDS; work-item t owns row py0 + t and walks ALL points of the item -- every lane reads the same address -- counting, up to 255, the hits of each
// pixel of its row: min(255, bg + k line) is the same for every k >= 255, as line is 0 or at least 1.  One barrier, then the rows are coloured and
// stored 4 pixels to a work-item.
CSDR_KERNEL_TRACE __launch_bounds__(kTrThreads) void trace_xy(TraceArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint8_t *hits = reinterpret_cast<uint8_t *>(smem);   // [rows_per][wp]
    const int tid = (int)threadIdx.x;
    const TraceTile tl = a.tiles[blockIdx.x];
    const int py0 = (int)blockIdx.y * a.rows_per, nr = min(a.rows_per, a.height - py0), groups = a.wp / 4;
    for (int i = tid; i < nr * groups; i += kTrThreads) reinterpret_cast<uint32_t *>(hits)[i] = 0u;
    __syncthreads();
    if (tid < nr) {
        uint8_t *mine = hits + (size_t)tid * a.wp;
        const int row = py0 + tid, np = tl.n / 2;
        for (int k = 0; k < np; ++k) {
            if (a.height - 1 - trace_quant(tl.pts[2 * (int64_t)k + 1], -1.0f, 0.5f, a.height) != row) continue;
            const int cx = trace_quant(tl.pts[2 * (int64_t)k], -1.0f, 0.5f, a.width);
            const uint8_t h = mine[cx];
            if (h < 255) mine[cx] = (uint8_t)(h + 1);
        }
    }
    __syncthreads();
    const uint32_t alpha = a.col.bg & 0xff000000u;
    for (int i = tid; i < nr * groups; i += kTrThreads) {
        const int r = i / groups, px0 = 4 * (i - r * groups);
        const uint32_t h4 = reinterpret_cast<const uint32_t *>(hits)[i];
        uint32_t px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t h = (h4 >> (8 * k)) & 0xffu;
            uint32_t v = alpha;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v |= min(255u, ((a.col.bg >> (8 * ch)) & 0xffu) + h * ((a.col.line >> (8 * ch)) & 0xffu)) << (8 * ch);
            px[k] = v;
        }
        wf_store4(a.out, trace_pixel(a, tl.tile, py0 + r, px0), min(4, a.width - px0), px[0], px[1], px[2], px[3]);
    }
}

}  // namespace csdr
