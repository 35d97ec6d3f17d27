// csdr_tracebank.hip -- implementation of include/csdr_hip.h (gfx950): csdr_tracebank, the spectrum, hold and scope lines of any number of items
// drawn as tiles of one RGBA8 atlas with the geometry of csdr_wfbank_render.  The object holds no signal state: a render checks its items, stages
// the host ones behind the tile records in ONE upload, and launches trace_lines once for all line kinds and empty tiles and trace_xy once for all XY
// items (kernels_tracebank.hpp).  The rule both follow is trace_host.hpp; csdr_design_trace_envelope is that rule on the host.  All work runs on a
// stream of the object's own (stream_order.hpp); device points are ordered behind the boundary stream by an event.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#define CSDR_TU_TRACEBANK 1  // this unit is the home of its kernels (kernels_tracebank.hpp)
#include "csdr_objects.hpp"
#include "kernels_tracebank.hpp"

using namespace csdr;

static_assert(sizeof(csdr_trace_item) == 32 && offsetof(csdr_trace_item, hold) == 8 && offsetof(csdr_trace_item, n) == 16 &&
              offsetof(csdr_trace_item, is_dev) == 28, "csdr_trace_item layout");

namespace {
constexpr int kTbStage = 2;                              // page-locked staging sets of the records and the staged points
constexpr int kTbTargetGroups = 2048;                    // trace_lines: workgroups to aim for before a tile's rows stay in one workgroup
uint32_t rgb_word(const uint8_t *c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }
}  // namespace

struct csdr_tracebank : SideStream {                     // (ev_in: device points of the caller; ev_out: csdr_tracebank_device_view)
    bool ready = false;
    int max_items = 0, max_points = 0;
    TraceColors col{0xff000000u, 0x00ffffffu, 0x0000ff00u, 0x00ffffffu, 0x00595959u};    // black / 255, white, (0, 255, 0), white, (89, 89, 89)
    DevBuf<uint32_t> view;                               // the last rendered atlas
    int view_w = 0, view_h = 0;                          // in pixels; 0: none
    StageRing<kTbStage> plan;                            // the tile records of the call being run and the staged host points behind them
};

#define TRB_LAUNCH(t_, kid_, kern_, grid_, lds_, ...) \
    do { ProfScope ps__((t_)->ctx, (kid_), (t_)->st); hipLaunchKernelGGL(kern_, grid_, dim3((unsigned)kTrThreads), lds_, (t_)->st, __VA_ARGS__); } while (0)

extern "C" int csdr_design_trace_envelope(const float *points, const float *hold, int n, int layout, int kind, int width, int height, int32_t *lo, int32_t *hi) {
    return trace_envelope(points, hold, n, layout, kind, width, height, lo, hi);
}

extern "C" int csdr_tracebank_create(csdr_ctx *ctx, csdr_tracebank **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    std::unique_ptr<csdr_tracebank, void (*)(csdr_tracebank *)> t(new csdr_tracebank(), csdr_tracebank_destroy);
    if (int rc = t->create(ctx)) return rc;
    if (int rc = t->plan.create()) return rc;
    *out = t.release();
    return CSDR_OK;
}

extern "C" void csdr_tracebank_destroy(csdr_tracebank *t) {
    DeviceScope dev__(t ? t->ctx : nullptr);
    if (!t) return;
    t->destroy();
    t->plan.destroy();
    t->view.release();
    delete t;
}

extern "C" int csdr_tracebank_setup(csdr_tracebank *t, int max_items, int max_points) {
    DeviceScope dev__(t ? t->ctx : nullptr);
    if (!t) return fail(CSDR_EINVAL, "trace bank is null");
    if (max_items < 1 || max_items > kTraceMaxItems) return fail(CSDR_EINVAL, "max_items %d: 1 .. 2^20", max_items);
    if (max_points < 1 || max_points > kTraceMaxPoints) return fail(CSDR_EINVAL, "max_points %d: 1 .. 2^21", max_points);
    CSDR_HIP_TRY(hipStreamSynchronize(t->st));
    t->max_items = max_items; t->max_points = max_points;
    t->view_w = t->view_h = 0;
    t->ready = true;
    return CSDR_OK;
}

// a null pointer leaves that colour as it is; the colours are kernel arguments of the next render, nothing is uploaded
extern "C" int csdr_tracebank_set_colors(csdr_tracebank *t, const uint8_t *bg, const uint8_t *line, const uint8_t *hold, const uint8_t *axis_major,
                                         const uint8_t *axis_minor) {
    if (!t) return fail(CSDR_EINVAL, "trace bank is null");
    if (bg) t->col.bg = rgb_word(bg) | ((uint32_t)bg[3] << 24);
    if (line) t->col.line = rgb_word(line);
    if (hold) t->col.hold = rgb_word(hold);
    if (axis_major) t->col.major = rgb_word(axis_major);
    if (axis_minor) t->col.minor = rgb_word(axis_minor);
    return CSDR_OK;
}

extern "C" int csdr_tracebank_render(csdr_tracebank *t, const csdr_trace_item *items, int n_items, int width, int height, int atlas_cols,
                                     uint8_t *out_u8, int64_t cap) {
    DeviceScope dev__(t ? t->ctx : nullptr);
    if (!t || !t->ready) return fail(CSDR_ESTATE, "trace bank not set up");
    if (int rc = trace_check_tile(width, height)) return rc;
    if (n_items < 1 || n_items > t->max_items || !items) return fail(CSDR_EINVAL, "n_items %d: 1 .. max_items (%d), no null pointer", n_items, t->max_items);
    if (atlas_cols < 1 || atlas_cols > n_items) return fail(CSDR_EINVAL, "atlas_cols %d: 1 .. n_items (%d)", atlas_cols, n_items);
    // ---- count: a refused call renders nothing and changes nothing
    size_t host_floats = 0, n_xy = 0;
    bool any_dev = false;
    auto drawn = [](const csdr_trace_item &it) { return it.n > 0 && it.points != nullptr; };
    for (int i = 0; i < n_items; ++i) {
        const csdr_trace_item &it = items[i];
        if (int rc = trace_check_item(it.kind, it.layout, it.n, height)) return rc;
        if (it.is_dev & ~(CSDR_TRACE_DEV_POINTS | CSDR_TRACE_DEV_HOLD)) return fail(CSDR_EINVAL, "item %d: is_dev %d", i, it.is_dev);
        if (it.n > t->max_points) return fail(CSDR_ERANGE, "item %d: n %d exceeds max_points %d", i, it.n, t->max_points);
        if (!drawn(it)) continue;
        const bool hold = it.kind == CSDR_TRACE_SPECTRUM && it.hold;
        if (((it.is_dev & CSDR_TRACE_DEV_POINTS) && ((uintptr_t)it.points & 3)) || (hold && (it.is_dev & CSDR_TRACE_DEV_HOLD) && ((uintptr_t)it.hold & 3)))
            return fail(CSDR_EINVAL, "item %d: device points must be 4-byte aligned", i);
        const size_t nf = (trace_item_floats(it.kind, it.layout, it.n) + 3) / 4 * 4;     // a staged polyline starts on a 16-byte boundary
        if (!(it.is_dev & CSDR_TRACE_DEV_POINTS)) host_floats += nf;
        if (hold && !(it.is_dev & CSDR_TRACE_DEV_HOLD)) host_floats += nf;
        if ((it.is_dev & CSDR_TRACE_DEV_POINTS) || (hold && (it.is_dev & CSDR_TRACE_DEV_HOLD))) any_dev = true;
        if (it.kind == CSDR_TRACE_SCOPE_XY) ++n_xy;
    }
    const int tile_rows = (n_items + atlas_cols - 1) / atlas_cols;
    const int64_t n_tiles = (int64_t)tile_rows * atlas_cols, n_lines = n_tiles - (int64_t)n_xy;
    const int64_t pic_w = (int64_t)atlas_cols * width, pic_h = (int64_t)tile_rows * height, pixels = pic_w * pic_h;
    const int col_blocks = (width + kTrCols - 1) / kTrCols;
    if (pic_w > 0x7fffffff || pic_h > 0x7fffffff || n_tiles * col_blocks > 0x7fffffff) return fail(CSDR_EINVAL, "an atlas of %lld x %lld pixels", (long long)pic_w, (long long)pic_h);
    if (out_u8 && cap < 4 * pixels) return fail(CSDR_ERANGE, "need %lld bytes", (long long)(4 * pixels));
    // ---- from here on only the device can refuse
    if ((size_t)pixels > t->view.cap) {
        CSDR_HIP_TRY(hipStreamSynchronize(t->st));
        t->view_w = t->view_h = 0;                       // (the buffer csdr_tracebank_device_view handed out goes away)
    }
    if (int rc = t->view.reserve((size_t)pixels)) return rc;
    const size_t points_at = (size_t)n_tiles * sizeof(TraceTile), bytes = points_at + host_floats * sizeof(float);
    if (int rc = t->plan.begin(t->st, bytes)) return rc;
    if (any_dev) if (int rc = t->after_boundary()) return rc;                    // the caller produced them on the boundary stream
    TraceTile *line_tiles = reinterpret_cast<TraceTile *>(t->plan.host()), *xy_tiles = line_tiles + n_lines;
    float *stage_h = reinterpret_cast<float *>(t->plan.host() + points_at);
    const float *stage_d = reinterpret_cast<const float *>(t->plan.device() + points_at);
    size_t at = 0, nl = 0, nx = 0;
    auto place = [&](const float *p, bool is_dev, size_t nf) {                  // -> where the device reads the polyline
        if (is_dev) return p;
        memcpy(stage_h + at, p, nf * sizeof(float));
        const float *d = stage_d + at;
        at += (nf + 3) / 4 * 4;
        return d;
    };
    for (int64_t k = 0; k < n_tiles; ++k) {
        TraceTile tl{nullptr, nullptr, 0, 1, -1, (int32_t)k};                    // an empty item or an unused tile of the last tile row
        if (k < n_items && drawn(items[k])) {
            const csdr_trace_item &it = items[k];
            const size_t nf = trace_item_floats(it.kind, it.layout, it.n);
            tl.pts = place(it.points, (it.is_dev & CSDR_TRACE_DEV_POINTS) != 0, nf);
            if (it.kind == CSDR_TRACE_SPECTRUM && it.hold) tl.hold = place(it.hold, (it.is_dev & CSDR_TRACE_DEV_HOLD) != 0, nf);
            tl.n = it.n; tl.stride = 1 + it.layout; tl.kind = it.kind;
        }
        if (tl.kind == CSDR_TRACE_SCOPE_XY) xy_tiles[nx++] = tl; else line_tiles[nl++] = tl;
    }
    if (int rc = t->plan.uploaded(t->st, points_at + at * sizeof(float))) return rc;
    TraceArgs a{};
    a.out = t->view.p; a.width = width; a.height = height; a.atlas_cols = atlas_cols; a.col = t->col;
    if (nl) {
        // enough row groups to fill the device, kTrRows rows to a group at least: a workgroup repeats the envelope of its columns per group
        const int groups_max = (height + kTrRows - 1) / kTrRows;
        const int groups = (int)std::max<int64_t>(1, std::min<int64_t>(groups_max, kTbTargetGroups / ((int64_t)nl * col_blocks)));
        a.tiles = reinterpret_cast<const TraceTile *>(t->plan.device());
        a.col_blocks = col_blocks;
        a.rows_per = ((height + groups - 1) / groups + kTrRows - 1) / kTrRows * kTrRows;
        const dim3 grid((unsigned)(nl * (size_t)col_blocks), (unsigned)((height + a.rows_per - 1) / a.rows_per));
        TRB_LAUNCH(t, KID_TRACE_LINES, trace_lines, grid, 4 * kTrCols * sizeof(int), a);
    }
    if (nx) {
        a.tiles = reinterpret_cast<const TraceTile *>(t->plan.device()) + n_lines;
        a.wp = (width + 3) / 4 * 4;
        a.rows_per = std::max(1, std::min(std::min(height, kTrThreads), kTrXyLds / a.wp));
        const dim3 grid((unsigned)nx, (unsigned)((height + a.rows_per - 1) / a.rows_per));
        TRB_LAUNCH(t, KID_TRACE_XY, trace_xy, grid, (size_t)a.rows_per * (size_t)a.wp, a);
    }
    CSDR_HIP_TRY(hipGetLastError());
    t->view_w = (int)pic_w; t->view_h = (int)pic_h;
    if (out_u8) {
        CSDR_HIP_TRY(hipMemcpyAsync(out_u8, t->view.p, (size_t)(4 * pixels), hipMemcpyDeviceToHost, t->st));
        CSDR_HIP_TRY(hipStreamSynchronize(t->st));
    }
    return CSDR_OK;
}

extern "C" int csdr_tracebank_device_view(csdr_tracebank *t, const uint8_t **dev, int *pic_width, int *pic_height) {
    DeviceScope dev__(t ? t->ctx : nullptr);
    if (!t || !dev) return fail(CSDR_EINVAL, "null argument");
    if (!t->ready || t->view_w == 0) return fail(CSDR_ESTATE, "nothing rendered yet (csdr_tracebank_render)");
    if (int rc = t->hand_over()) return rc;
    *dev = reinterpret_cast<const uint8_t *>(t->view.p);
    if (pic_width) *pic_width = t->view_w;
    if (pic_height) *pic_height = t->view_h;
    return CSDR_OK;
}
