// trace_host.hpp -- the drawing rule of csdr_tracebank (include/csdr_hip.h, "Trace bank"), stated once: the quantiser, the column of a vertex, the
// rows a segment gives a column, which polylines a kind draws and where its axis rows lie.  The kernels (kernels_tracebank.hpp) call these very
// functions on the device; csdr_design_trace_envelope (trace_envelope below) and the object's argument checks call them on the host.  After the one
// float step per vertex (trace_quant) everything is integer arithmetic whose values fit 32 bits for every size the checks admit -- rows and columns
// below 2^14, t <= 2^15 -- except the products i * W and c * n, which are 64-bit.
#pragma once
#include <climits>

#include "common.hpp"

namespace csdr {

constexpr int kTraceMaxSide = 16384, kTraceMaxItems = 1 << 20, kTraceMaxPoints = 1 << 21;

// u = (y - y0) * s, each operation rounded to float on its own (no product-sum in it that could be contracted); q = floor(u * N) in [0, N - 1].
// u <= 0, -0.0 and NaN give 0 (the library's own definition, as the waterfall quantiser's); u >= 1 and +inf give N - 1.
__host__ __device__ inline int trace_quant(float y, float y0, float s, int N) {
    const float u = (y - y0) * s;
    if (!(u > 0.0f)) return 0;
    if (u >= 1.0f) return N - 1;
    const int q = (int)floorf(u * (float)N);
    return q < 0 ? 0 : (q > N - 1 ? N - 1 : q);
}

// rdiv(p, q) = floor((2 p + q) / (2 q)), q > 0: p / q rounded to the nearest integer, halves upwards, for negative p too
__host__ __device__ inline int trace_rdiv(int p, int q) {
    const int num = 2 * p + q, den = 2 * q;
    return num / den - (num % den < 0 ? 1 : 0);
}

// One polyline of an item inside its tile: n vertices, vertex i at p[i * stride + stride - 1]; a panel of hp rows starting at tile row r0 with
// the quantiser constants (y0, s).  n == 0: this polyline is not drawn.
struct TracePoly {
    const float *p;
    int n, stride, hp, r0;
    float y0, s;
};
// which = 0: the line (2Y: the upper sub-panel's); which = 1: the hold points of a spectrum, the lower sub-panel's line of 2Y, nothing otherwise
__host__ __device__ inline TracePoly trace_poly(const float *points, const float *hold, int n, int stride, int kind, int H, int which) {
    TracePoly pl{points, n, stride, H, 0, 0.0f, 1.0f};
    if (kind == CSDR_TRACE_SPECTRUM) {
        if (which) { pl.p = hold; if (!hold) pl.n = 0; }
        return pl;
    }
    pl.y0 = -1.0f; pl.s = 0.5f;
    if (kind == CSDR_TRACE_SCOPE_2Y) {
        const int m = n / 2, hu = H / 2;                 // (an odd last vertex is not drawn)
        pl.n = m;
        if (which) { pl.p = points + (int64_t)m * stride; pl.hp = H - hu; pl.r0 = hu; } else pl.hp = hu;
        return pl;
    }
    if (which) pl.n = 0;
    return pl;
}
__host__ __device__ inline bool trace_hold_blends(int kind) { return kind == CSDR_TRACE_SPECTRUM; }     // which = 1 is averaged over what lies under it

// the tile row of vertex i: row 0 is the top of the panel
__host__ __device__ inline int trace_row(const TracePoly &pl, int64_t i) {
    return pl.r0 + pl.hp - 1 - trace_quant(pl.p[i * pl.stride + (pl.stride - 1)], pl.y0, pl.s, pl.hp);
}
// vertices [v0, v1) lie in column c: c_i = floor(i W / n) = c  <=>  ceil(c n / W) <= i < ceil((c + 1) n / W)
__host__ __device__ inline int64_t trace_first_vertex(int64_t c, int n, int W) { return (c * n + W - 1) / W; }

// what segment (i, i + 1) gives column c, a = c_i <= c <= b = c_{i+1}, a < b: the two rows at t = clamp(2 (c - a) -+ 1, 0, 2 d)
__host__ __device__ inline void trace_segment(const TracePoly &pl, int W, int c, int64_t i, int &lo, int &hi) {
    const int a = (int)(i * W / pl.n), b = (int)((i + 1) * W / pl.n), d = b - a;
    if (d <= 0) return;
    const int ra = trace_row(pl, i), rb = trace_row(pl, i + 1);
    for (int k = -1; k <= 1; k += 2) {
        int t = 2 * (c - a) + k;
        t = t < 0 ? 0 : (t > 2 * d ? 2 * d : t);
        const int r = ra + trace_rdiv((rb - ra) * t, 2 * d);
        lo = r < lo ? r : lo; hi = r > hi ? r : hi;
    }
}
// lo / hi hold the hull of the rows of the column's own vertices [v0, v1) (INT_MAX / -1: none).  Added here: the segment that enters the column
// (or, where the column has no vertex, crosses it) and the one that leaves it.  Segments between two vertices of one column add nothing.
__host__ __device__ inline void trace_neighbours(const TracePoly &pl, int W, int c, int64_t v0, int64_t v1, int &lo, int &hi) {
    if (v0 > 0 && v0 < pl.n) trace_segment(pl, W, c, v0 - 1, lo, hi);
    if (v1 > v0 && v1 < pl.n) trace_segment(pl, W, c, v1 - 1, lo, hi);
}

// the axis rows of a tile, -1: none.  Paint order: background, minor rows, major row, line, hold
struct TraceAxes { int minor0, minor1, major; };
__host__ __device__ inline TraceAxes trace_axes(int kind, int H) {
    TraceAxes ax{-1, -1, -1};
    if (kind == CSDR_TRACE_SCOPE_Y) ax.minor0 = H - 1 - trace_quant(0.0f, -1.0f, 0.5f, H);
    else if (kind == CSDR_TRACE_SCOPE_2Y) {
        const int hu = H / 2, hl = H - hu;
        ax.minor0 = hu - 1 - trace_quant(0.0f, -1.0f, 0.5f, hu);
        ax.minor1 = hu + hl - 1 - trace_quant(0.0f, -1.0f, 0.5f, hl);
        ax.major = hu;
    }
    return ax;
}

// ---- host only: the checks the object and the design call share, and the rule column by column ----
inline int trace_check_tile(int width, int height) {
    if (width < 2 || width > kTraceMaxSide || height < 1 || height > kTraceMaxSide)
        return fail(CSDR_EINVAL, "a tile of %d x %d (width 2 .. 16384, height 1 .. 16384)", width, height);
    return CSDR_OK;
}
inline int trace_check_item(int kind, int layout, int n, int height) {
    if (kind < CSDR_TRACE_SPECTRUM || kind > CSDR_TRACE_SCOPE_XY) return fail(CSDR_EINVAL, "kind %d: 0 .. 3", kind);
    if (layout != 0 && layout != 1) return fail(CSDR_EINVAL, "layout %d: 0 | 1", layout);
    if (n < 0) return fail(CSDR_EINVAL, "n %d is negative", n);
    if (kind == CSDR_TRACE_SCOPE_2Y && height < 2) return fail(CSDR_EINVAL, "CSDR_TRACE_SCOPE_2Y needs two rows");
    return CSDR_OK;
}
// floats an item's `points` (and `hold`) hold: XY counts floats, the line kinds count vertices
inline size_t trace_item_floats(int kind, int layout, int n) { return kind == CSDR_TRACE_SCOPE_XY ? (size_t)n : (size_t)n * (size_t)(1 + layout); }

inline int trace_envelope(const float *points, const float *hold, int n, int layout, int kind, int width, int height, int32_t *lo, int32_t *hi) {
    if (!lo || !hi) return fail(CSDR_EINVAL, "null argument");
    if (int rc = trace_check_tile(width, height)) return rc;
    if (int rc = trace_check_item(kind, layout, n, height)) return rc;
    if (kind == CSDR_TRACE_SCOPE_XY) return fail(CSDR_EINVAL, "CSDR_TRACE_SCOPE_XY draws points: it has no envelope");
    if (n > kTraceMaxPoints) return fail(CSDR_ERANGE, "n %d: 2^21 at most", n);
    if (n > 0 && !points) return fail(CSDR_EINVAL, "null points");
    for (int which = 0; which < 2; ++which) {
        const TracePoly pl = trace_poly(points, hold, n, 1 + layout, kind, height, which);
        for (int c = 0; c < width; ++c) {
            int l = INT_MAX, h = -1;
            if (pl.n > 0) {
                const int64_t v0 = trace_first_vertex(c, pl.n, width), v1 = trace_first_vertex((int64_t)c + 1, pl.n, width);
                for (int64_t i = v0; i < v1; ++i) { const int r = trace_row(pl, i); l = r < l ? r : l; h = r > h ? r : h; }
                trace_neighbours(pl, width, c, v0, v1, l, h);
            }
            lo[(size_t)which * width + c] = h < 0 ? -1 : l;
            hi[(size_t)which * width + c] = h;
        }
    }
    return CSDR_OK;
}

}  // namespace csdr
