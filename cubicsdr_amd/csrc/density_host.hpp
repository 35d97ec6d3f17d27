// density_host.hpp -- the rule of csdr_density (include/csdr_hip.h, "Density bank"), stated once: the interval a frame lights in a column, the step
// of a cell and the palette index of a count.  The kernels (kernels_density.hpp) call these very functions on the device; the object's argument
// checks and csdr_design_density_cover (density_cover_host below) call them on the host.  The interval is the trace bank's: trace_quant,
// trace_first_vertex, trace_row and trace_neighbours of trace_host.hpp are called as they are, nothing of them is restated here.
#pragma once
#include "kernels_waterfall.hpp"             // HideDcSpan, hide_dc_source
#include "trace_host.hpp"

namespace csdr {

constexpr int kDnMaxWidth = 16384, kDnMaxHeight = 2048, kDnMaxFrames = 1 << 20, kDnMaxViews = 1 << 20;
constexpr int64_t kDnMaxCells = (int64_t)1 << 30;
constexpr uint32_t kDnMaxKeep = 65536u, kDnMaxWeight = 1u << 24;

// the y of vertex i of a polyline, where trace_row reads it
__host__ __device__ inline float density_y(const TracePoly &pl, int64_t i) { return pl.p[i * pl.stride + (pl.stride - 1)]; }

// The segment (x - 1, x) as trace_neighbours adds it, with the DC-spike overwrite applied to its two vertices: their values are put into `win`
// (two floats of the caller's: a work-item's own LDS on the device, the stack on the host) and trace_neighbours is called on a polyline of stride
// 1 whose vertices x - 1 and x are those two floats.  With v0 == v1 == x it adds the segment that enters x's column and nothing else.
__host__ __device__ inline void density_edge(const TracePoly &pl, const HideDcSpan &dc, int W, int c, int64_t x, float *win, int &lo, int &hi) {
    if (x <= 0 || x >= pl.n) return;
    win[0] = density_y(pl, hide_dc_source(dc, (int)(x - 1)));
    win[1] = density_y(pl, hide_dc_source(dc, (int)x));
    TracePoly w = pl;
    w.p = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(win) - (uintptr_t)(x - 1) * sizeof(float));      // w.p[x - 1] is win[0]
    w.stride = 1;
    trace_neighbours(w, W, c, x, x, lo, hi);
}

// item 1: the interval [lo, hi] frame `pl` lights in column c, whose own vertices are [v0, v1) (trace_first_vertex); hi = -1: unlit.  Vertex i
// reads the point hide_dc_source(dc, i).  The two calls of density_edge are trace_neighbours(pl, W, c, v0, v1, ..) taken apart: the segment
// that enters the column (or crosses it) and, where the column has a vertex, the one that leaves it.
__host__ __device__ inline void density_interval(const TracePoly &pl, const HideDcSpan &dc, int W, int c, int64_t v0, int64_t v1, float *win, int &lo, int &hi) {
    lo = INT_MAX; hi = -1;
    for (int64_t i = v0; i < v1; ++i) { const int r = trace_row(pl, hide_dc_source(dc, (int)i)); lo = r < lo ? r : lo; hi = r > hi ? r : hi; }
    density_edge(pl, dc, W, c, v0, win, lo, hi);
    if (v1 > v0) density_edge(pl, dc, W, c, v1, win, lo, hi);
}

// item 2: one cell's step, in 64 bits
__host__ __device__ inline uint32_t density_step_cell(uint32_t count, uint32_t keep_q16, uint32_t weight, uint32_t cover) {
    const uint64_t v = (((uint64_t)count * keep_q16) >> 16) + (uint64_t)weight * cover;
    return v > 0xffffffffull ? 0xffffffffu : (uint32_t)v;
}
// item 4: the palette index of a count; full_eff >= 1
__host__ __device__ inline uint32_t density_index(uint32_t count, uint32_t full_eff) {
    if (count == 0) return 0;
    if (count >= full_eff) return 255;
    const uint32_t q = (uint32_t)((uint64_t)count * 255u / full_eff);
    return q < 1 ? 1 : q;
}

// ---- host only: the checks the object and the design call share, and item 1 frame by frame ----
inline int density_check_tile(int width, int height) {
    if (width < 2 || width > kDnMaxWidth || height < 1 || height > kDnMaxHeight)
        return fail(CSDR_EINVAL, "a tile of %d x %d (width 2 .. 16384, height 1 .. 2048)", width, height);
    return CSDR_OK;
}
inline bool density_item_reads(const float *points, int n, int frames) { return points != nullptr && n > 0 && frames > 0; }
inline int density_check_frames(const float *points, int n, int layout, int64_t stride_floats, int frames, int kind) {
    if (kind != CSDR_TRACE_SPECTRUM && kind != CSDR_TRACE_SCOPE_Y) return fail(CSDR_EINVAL, "kind %d: CSDR_TRACE_SPECTRUM | CSDR_TRACE_SCOPE_Y", kind);
    if (layout != 0 && layout != 1) return fail(CSDR_EINVAL, "layout %d: 0 | 1", layout);
    if (n < 0 || frames < 0) return fail(CSDR_EINVAL, "n %d, frames %d: neither may be negative", n, frames);
    if (density_item_reads(points, n, frames) && stride_floats < (int64_t)n * (1 + layout))
        return fail(CSDR_EINVAL, "stride_floats %lld is below n * (1 + layout) = %lld", (long long)stride_floats, (long long)n * (1 + layout));
    return CSDR_OK;
}

inline int density_cover_host(const float *points, int n, int layout, int64_t stride_floats, int frames, int kind, int width, int height, uint32_t *cover) {
    if (!cover) return fail(CSDR_EINVAL, "null argument");
    if (int rc = density_check_tile(width, height)) return rc;
    if (int rc = density_check_frames(points, n, layout, stride_floats, frames, kind)) return rc;
    if (n > kTraceMaxPoints) return fail(CSDR_ERANGE, "n %d: 2^21 at most", n);
    if (frames > kDnMaxFrames) return fail(CSDR_ERANGE, "frames %d: 2^20 at most", frames);
    memset(cover, 0, (size_t)width * (size_t)height * sizeof(uint32_t));
    if (!density_item_reads(points, n, frames)) return CSDR_OK;
    const HideDcSpan none;
    for (int f = 0; f < frames; ++f) {
        const TracePoly pl = trace_poly(points + (int64_t)f * stride_floats, nullptr, n, 1 + layout, kind, height, 0);
        for (int c = 0; c < width; ++c) {
            float win[2];
            int lo, hi;
            density_interval(pl, none, width, c, trace_first_vertex(c, n, width), trace_first_vertex((int64_t)c + 1, n, width), win, lo, hi);
            for (int r = lo; r <= hi; ++r) ++cover[(size_t)r * width + c];
        }
    }
    return CSDR_OK;
}

}  // namespace csdr
