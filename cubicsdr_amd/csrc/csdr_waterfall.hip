// csdr_waterfall.hip -- implementation of include/csdr_hip.h (gfx950): csdr_waterfall (WaterfallPanel, src/panel/WaterfallPanel.cpp, with the
// gradient of src/util/Gradient.cpp).  Host-side bookkeeping mirrors the panel's control flow (file:line cited per function); the bytes are moved
// by the kernels of kernels_waterfall.hpp.  All work of one waterfall is enqueued on a stream of its own, so a display consumer never holds up a
// lane of the pipeline; a spectrum's points are reached through spec_points_acquire / _release (csdr_objects.hpp), ordered by events.
#include <algorithm>
#include <memory>
#include <vector>

#define CSDR_TU_WATERFALL 1     // this unit is the home of its kernels (kernels_waterfall.hpp)
#include "csdr_objects.hpp"
#include "waterfall_host.hpp"

using namespace csdr;

struct csdr_waterfall : SideStream {                   // (ev_in: device points of the caller; ev_out: csdr_waterfall_device_rgba)
    bool ready = false;
    int fft_size = 0, half = 0, pitch = 0, lines = 0, max_pending = 0;
    // WaterfallPanel's state
    int lines_buffered = 0;                            // lines_buffered (:16, :81, :157)
    bool buffer_init = false, tex_init = false;        // bufferInitialized, texInitialized (:22-23)
    int ofs[2] = {0, 0};                               // waterfall_ofs
    DevBuf<float> points, stage;                       // `points` (:18-20, :39-49); staging of host lines
    DevBuf<uint8_t> pend, ring;                        // lineBuffer[2]: [2][max_pending][pitch]; the two textures: [2][lines][pitch]
    DevBuf<uint32_t> table, image;                     // the 256-entry RGBA8 table; the last rendered picture
    int64_t image_pixels = 0;
    // the viewport (csdr_waterfall_render_view): tap tables per (geometry, width, height, mode) -- they do not depend on ofs -- and a picture of its own
    WfTapCache taps;
    DevBuf<uint32_t> view;
    int view_w = 0, view_h = 0;                        // the last rendered view; 0: none
    int peak_tile[2] = {0, 0}, peak_slots = 0;         // wf_view_peak's tiling for `taps`
    uint8_t *pend_of(int j) const { return pend.p + (size_t)j * max_pending * pitch; }
    uint8_t *ring_of(int j) const { return ring.p + (size_t)j * lines * pitch; }
};

#define WF_LAUNCH(w_, kid_, kern_, grid_, lds_, ...) \
    do { ProfScope ps__((w_)->ctx, (kid_), (w_)->st); hipLaunchKernelGGL(kern_, grid_, dim3(kWfThreads), lds_, (w_)->st, __VA_ARGS__); } while (0)

extern "C" int csdr_waterfall_create(csdr_ctx *ctx, csdr_waterfall **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    std::unique_ptr<csdr_waterfall, void (*)(csdr_waterfall *)> w(new csdr_waterfall(), csdr_waterfall_destroy);
    if (int rc = w->create(ctx)) return rc;
    if (int rc = w->table.reserve(256)) return rc;
    if (int rc = wf_upload_grey_table(w->st, w->table.p)) return rc;        // before any csdr_waterfall_set_gradient
    *out = w.release();
    return CSDR_OK;
}

extern "C" void csdr_waterfall_destroy(csdr_waterfall *w) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w) return;
    w->destroy();
    w->points.release(); w->stage.release(); w->pend.release(); w->ring.release(); w->table.release(); w->image.release(); w->taps.dev.release(); w->view.release();
    delete w;
}

// WaterfallPanel::setup (:13-24)
extern "C" int csdr_waterfall_setup(csdr_waterfall *w, int fft_size, int lines, int max_pending) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w) return fail(CSDR_EINVAL, "waterfall is null");
    if (fft_size < 2 || fft_size > (1 << 21)) return fail(CSDR_EINVAL, "fft_size %d", fft_size);
    // (with one line waterfall_ofs starts at 0, the first run has no rows and the loop of :140-158 never ends)
    if (lines < 2 || lines > (1 << 20)) return fail(CSDR_EINVAL, "lines %d: 2 .. 2^20", lines);
    if (max_pending < 1 || max_pending > (1 << 20)) return fail(CSDR_EINVAL, "max_pending %d: 1 .. 2^20", max_pending);
    CSDR_HIP_TRY(hipStreamSynchronize(w->st));
    const int half = fft_size / 2, pitch = (half + 15) / 16 * 16;
    if (fft_size != w->fft_size) {                       // points.resize(fft_size) (:18-20): the values in front stay, new ones are zero
        DevBuf<float> np;
        if (int rc = np.reserve((size_t)fft_size)) return rc;
        CSDR_HIP_TRY(hipMemsetAsync(np.p, 0, (size_t)fft_size * sizeof(float), w->st));
        if (w->fft_size > 0) CSDR_HIP_TRY(hipMemcpyAsync(np.p, w->points.p, (size_t)std::min(fft_size, w->fft_size) * sizeof(float), hipMemcpyDeviceToDevice, w->st));
        CSDR_HIP_TRY(hipStreamSynchronize(w->st));
        w->points.release();
        w->points = np;
    }
    w->ready = false;
    if (int rc = w->pend.reserve((size_t)2 * max_pending * pitch)) return rc;
    if (int rc = w->ring.reserve((size_t)2 * lines * pitch)) return rc;
    CSDR_HIP_TRY(hipMemsetAsync(w->pend.p, 0, (size_t)2 * max_pending * pitch, w->st));       // (the rows' padding is copied along by wf_update: keep it defined)
    w->fft_size = fft_size; w->half = half; w->pitch = pitch; w->lines = lines; w->max_pending = max_pending;
    w->lines_buffered = 0;                               // :16
    w->tex_init = false; w->buffer_init = false;         // :22-23
    w->image_pixels = 0;
    w->taps.forget(); w->view_w = w->view_h = 0;
    w->ready = true;
    return CSDR_OK;
}

// Gradient::generate(len) (Gradient.cpp:37-85); host only
extern "C" int csdr_design_gradient(const float *rgb_stops, int n_colors, int len, float *r, float *g, float *b) {
    if (!design::gradient(rgb_stops, n_colors, len, r, g, b)) return fail(CSDR_EINVAL, "gradient: %d stops for %d entries (2 .. len + 1 stops, no null pointer)", n_colors, len);
    return CSDR_OK;
}

// refreshTheme (:26-37): the three 256-entry pixel maps, as one RGBA8 table
extern "C" int csdr_waterfall_set_gradient(csdr_waterfall *w, const float *rgb_stops, int n_colors) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w) return fail(CSDR_EINVAL, "waterfall is null");
    uint32_t t[256];
    if (!design::gradient_rgba8(rgb_stops, n_colors, t)) return fail(CSDR_EINVAL, "gradient: %d stops (2 .. 257, no null pointer)", n_colors);
    return wf_upload_table(w->st, w->table.p, t);
}

// setPoints (:39-49) + step (:51-83) for n_lines lines that lie at src (device memory, ordered on w->st); valid = 0: the previous points, n_lines times
static int wf_step(csdr_waterfall *w, const float *src, int64_t line_stride, int pair, int valid, int n_lines, const HideDcSpan &dc, int *taken) {
    if (taken) *taken = 0;
    if (n_lines == 0) return CSDR_OK;
    const bool drop = !w->tex_init;                      // :60-62
    if (!drop && w->lines_buffered + (int64_t)n_lines > w->max_pending)
        return fail(CSDR_ERANGE, "%d pending lines + %d exceed max_pending %d", w->lines_buffered, n_lines, w->max_pending);
    w->buffer_init = true;                               // :54-58
    if (drop && !valid) return CSDR_OK;                  // nothing to quantise, nothing to keep
    WfQuantArgs a{};
    a.half = w->half; a.pitch = w->pitch;
    a.pend[0] = w->pend_of(0); a.pend[1] = w->pend_of(1);
    a.row0 = w->lines_buffered; a.n_lines = n_lines; a.store = drop ? 0 : 1;
    if (valid) { a.src = src; a.line_stride = line_stride; a.pair = pair; a.keep = w->points.p; a.dc = dc; }
    else { a.src = w->points.p; a.line_stride = 0; a.pair = 0; a.keep = nullptr; }
    if (drop) { a.src += (int64_t)(n_lines - 1) * a.line_stride; a.n_lines = 1; }        // only the last line's values are kept
    a.wide = (w->half % 16 == 0) && (w->fft_size == 2 * w->half) && ((uintptr_t)a.src % 16 == 0) && (a.line_stride % 4 == 0);
    const int items = (w->half + kWfChunk - 1) / kWfChunk;
    const dim3 grid((unsigned)((items + kWfThreads - 1) / kWfThreads), (unsigned)std::min(a.n_lines, 65535), 2);
    WF_LAUNCH(w, KID_WF_QUANTIZE, wf_quantize, grid, 0, a);
    CSDR_HIP_TRY(hipGetLastError());
    if (!drop) { w->lines_buffered += n_lines; if (taken) *taken = n_lines; }             // :81
    return CSDR_OK;
}

extern "C" int csdr_waterfall_step(csdr_waterfall *w, const float *points, int is_dev, int n_floats_per_line, int n_lines, int *taken) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (taken) *taken = 0;
    if (!w || !w->ready) return fail(CSDR_ESTATE, "waterfall not set up");
    if (n_lines < 0 || n_floats_per_line < 0) return fail(CSDR_EINVAL, "bad line arguments");
    const int pair = wf_line_is_pairs(n_floats_per_line, w->fft_size) ? 1 : 0;
    const int valid = wf_good_line(points, n_floats_per_line, w->fft_size) ? 1 : 0;        // (a line of another length: the step repeats the points)
    const float *src = points;
    if (valid && n_lines > 0) {
        if (!w->tex_init || w->lines_buffered + (int64_t)n_lines <= w->max_pending) {      // (a refused call moves nothing)
            if (is_dev) {
                if ((uintptr_t)points & 3) return fail(CSDR_EINVAL, "device points must be 4-byte aligned");
                if (int rc = w->after_boundary()) return rc;                                 // the caller produced them on the boundary stream
            } else {
                const size_t n = (size_t)n_lines * (size_t)n_floats_per_line;
                if (n > w->stage.cap) CSDR_HIP_TRY(hipStreamSynchronize(w->st));             // (a kernel may still read the buffer being replaced)
                if (int rc = w->stage.reserve(n)) return rc;
                CSDR_HIP_TRY(hipMemcpyAsync(w->stage.p, points, n * sizeof(float), hipMemcpyHostToDevice, w->st));
                src = w->stage.p;
            }
        }
    }
    return wf_step(w, src, n_floats_per_line, pair, valid, n_lines, HideDcSpan(), taken);
}

extern "C" int csdr_waterfall_step_spec(csdr_waterfall *w, csdr_spec *spec, int frame0, int n_frames, int *taken) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (taken) *taken = 0;
    if (!w || !w->ready) return fail(CSDR_ESTATE, "waterfall not set up");
    if (!spec) return fail(CSDR_EINVAL, "spec is null");
    SpecPointsRef ref;
    if (int rc = spec_points_acquire(spec, w->st, &ref)) return rc;
    if (ref.ctx != w->ctx) return fail(CSDR_EINVAL, "the spectrum belongs to another context");
    if (frame0 < 0 || n_frames < 0 || frame0 + (int64_t)n_frames > ref.frames) return fail(CSDR_EINVAL, "frames %d .. %d of %d", frame0, frame0 + n_frames, ref.frames);
    // a spectrum of another size is a frame of the wrong size (WaterfallCanvas.cpp:106-109): the previous points are stepped
    const int valid = ref.F == w->fft_size ? 1 : 0;
    const int rc = wf_step(w, ref.points + (size_t)frame0 * ref.F, ref.F, 0, valid, n_frames, ref.dc, taken);
    if (int r2 = spec_points_release(spec, w->st)) return r2;
    return rc;
}

// WaterfallPanel::update (:85-159)
extern "C" int csdr_waterfall_update(csdr_waterfall *w) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !w->ready) return fail(CSDR_ESTATE, "waterfall not set up");
    if (!w->buffer_init) return CSDR_OK;                 // :88-90
    if (!w->tex_init) {                                  // :92-130: both textures zero-filled, waterfall_ofs = waterfall_lines - 1
        CSDR_HIP_TRY(hipMemsetAsync(w->ring.p, 0, (size_t)2 * w->lines * w->pitch, w->st));
        w->ofs[0] = w->ofs[1] = w->lines - 1;
        w->tex_init = true;
    }
    const int n = w->lines_buffered;
    if (n == 0) return CSDR_OK;
    const WfUpdatePlan plan = wf_plan_update(w->ofs[0], w->lines, n);             // :139-158
    WfUpdateArgs a{};
    a.run[0] = plan.run[0]; a.run[1] = plan.run[1]; a.n_runs = plan.n_runs;
    a.n_pending = n; a.pitch = w->pitch;
    for (int j = 0; j < 2; ++j) { a.ring[j] = w->ring_of(j); a.pend[j] = w->pend_of(j); }
    const int rows = plan.rows(), chunks = w->pitch / 16;
    const dim3 grid((unsigned)std::min((chunks + kWfThreads - 1) / kWfThreads, 64), (unsigned)std::min(rows, 65535), 2);
    WF_LAUNCH(w, KID_WF_UPDATE, wf_update, grid, 0, a);
    CSDR_HIP_TRY(hipGetLastError());
    w->ofs[0] = w->ofs[1] = plan.ofs;                    // (both offsets move together: they start equal)
    w->lines_buffered = 0;
    return CSDR_OK;
}

extern "C" int csdr_waterfall_lines_buffered(const csdr_waterfall *w) { return w && w->ready ? w->lines_buffered : 0; }
extern "C" int csdr_waterfall_offset(const csdr_waterfall *w, int half) { return w && w->ready && w->tex_init && (half == 0 || half == 1) ? w->ofs[half] : -1; }

extern "C" int csdr_waterfall_fetch_index(csdr_waterfall *w, int half, uint8_t *out_u8, int64_t cap) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !w->ready || !w->tex_init) return fail(CSDR_ESTATE, "no textures yet (setup, step, update)");
    if ((half != 0 && half != 1) || !out_u8) return fail(CSDR_EINVAL, "bad argument");
    if (cap < (int64_t)w->lines * w->half) return fail(CSDR_ERANGE, "need %lld bytes", (long long)w->lines * w->half);
    return wf_fetch_rows(w->st, w->ring_of(half), w->lines, w->half, w->pitch, out_u8);
}

// drawPanelContents (:161-219), unscaled
extern "C" int csdr_waterfall_fetch_rgba(csdr_waterfall *w, int first_row, int n_rows, uint8_t *out_u8, int64_t cap) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !w->ready || !w->tex_init) return fail(CSDR_ESTATE, "no textures yet (setup, step, update)");         // :162-164
    if (first_row < 0 || n_rows < 1 || first_row + (int64_t)n_rows > w->lines) return fail(CSDR_EINVAL, "rows %d + %d of %d", first_row, n_rows, w->lines);
    const int64_t pixels = (int64_t)n_rows * 2 * w->half;
    if (out_u8 && cap < 4 * pixels) return fail(CSDR_ERANGE, "need %lld bytes", (long long)(4 * pixels));
    if ((size_t)pixels > w->image.cap) CSDR_HIP_TRY(hipStreamSynchronize(w->st));
    if (int rc = w->image.reserve((size_t)pixels)) return rc;
    WfRgbaArgs a{};
    a.ring[0] = w->ring_of(0); a.ring[1] = w->ring_of(1); a.table = w->table.p; a.out = w->image.p;
    a.half = w->half; a.pitch = w->pitch; a.lines = w->lines; a.ofs = w->ofs[0]; a.first_row = first_row; a.n_rows = n_rows;
    const int groups = (w->half + 3) / 4;
    const dim3 grid((unsigned)((groups + kWfThreads - 1) / kWfThreads), (unsigned)std::min(n_rows, 65535), 2);
    WF_LAUNCH(w, KID_WF_RGBA, wf_rgba, grid, 256 * sizeof(uint32_t), a);
    CSDR_HIP_TRY(hipGetLastError());
    w->image_pixels = pixels;
    if (out_u8) {
        CSDR_HIP_TRY(hipMemcpyAsync(out_u8, w->image.p, (size_t)(4 * pixels), hipMemcpyDeviceToHost, w->st));
        CSDR_HIP_TRY(hipStreamSynchronize(w->st));
    }
    return CSDR_OK;
}

extern "C" int csdr_waterfall_device_rgba(csdr_waterfall *w, const uint8_t **dev) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !dev) return fail(CSDR_EINVAL, "null argument");
    if (!w->ready || w->image_pixels == 0) return fail(CSDR_ESTATE, "nothing rendered yet (csdr_waterfall_fetch_rgba)");
    if (int rc = w->hand_over()) return rc;
    *dev = reinterpret_cast<const uint8_t *>(w->image.p);
    return CSDR_OK;
}

// ---- the viewport: drawPanelContents (:161-219) scaled to width x height (csdr_hip.h, "Waterfall viewport") ----
static_assert(sizeof(design::ViewTap) == sizeof(csdr_view_tap) && offsetof(design::ViewTap, frac) == offsetof(csdr_view_tap, frac) &&
              offsetof(design::ViewTap, half) == offsetof(csdr_view_tap, half), "design::ViewTap is csdr_view_tap");

extern "C" int csdr_design_view_columns(int fft_size, int width, int mode, csdr_view_tap *taps) {
    if (!design::view_columns(fft_size, width, mode, reinterpret_cast<design::ViewTap *>(taps)))
        return fail(CSDR_EINVAL, "view columns: fft_size %d (>= 4), width %d (2 .. 16384), mode %d, no null pointer", fft_size, width, mode);
    return CSDR_OK;
}
extern "C" int csdr_design_view_rows(int lines, int height, int mode, csdr_view_tap *taps) {
    if (!design::view_rows(lines, height, mode, reinterpret_cast<design::ViewTap *>(taps)))
        return fail(CSDR_EINVAL, "view rows: lines %d (2 .. 2^20), height %d (1 .. 16384), mode %d, no null pointer", lines, height, mode);
    return CSDR_OK;
}

constexpr int kWfPeakSlots = 1024;           // 16 KB of LDS for a tile's texel span: nine workgroups to a compute unit

// the tap tables of (width, height, mode) on the device; for PEAK, when they are rebuilt, also the tiling: as many pixels to a workgroup (up to one
// per work-item) as keep the tile's span, widened to 16-byte chunks, inside the slots -- a single pixel wider than that is a tile of its own and is
// folded by the kernel
static int wf_view_tables(csdr_waterfall *w, int width, int height, int mode) {
    return w->taps.ensure(w->st, w->fft_size, w->lines, width, height, mode, [&](const csdr_view_tap *t) {
        int tile[2] = {0, 0}, slots = 1;
        if (mode == CSDR_WF_VIEW_PEAK) {
            const int n0 = width / 2;
            for (int h = 0; h < 2; ++h) {
                const int64_t nh = h ? width - n0 : n0;
                tile[h] = (int)std::max<int64_t>(1, std::min<int64_t>(kWfThreads, ((int64_t)kWfPeakSlots * 16 - 32) * nh / w->half));
                const csdr_view_tap *c = t + (h ? n0 : 0);
                for (int64_t k0 = 0; k0 < nh; k0 += tile[h]) {
                    const csdr_view_tap &a = c[k0], &b = c[std::min<int64_t>(k0 + tile[h], nh) - 1];
                    const int chunks = (b.first + b.count + 15) / 16 - a.first / 16;
                    if (chunks > kWfPeakSlots && tile[h] > 1) return fail(CSDR_EINVAL, "view tiling: %d chunks for %d pixels", chunks, tile[h]);
                    slots = std::max(slots, std::min(chunks, kWfPeakSlots));
                }
            }
        }
        w->peak_tile[0] = tile[0]; w->peak_tile[1] = tile[1]; w->peak_slots = slots;      // (read only while `taps` holds these tables)
        return (int)CSDR_OK;
    });
}

extern "C" int csdr_waterfall_render_view(csdr_waterfall *w, int width, int height, int mode, uint8_t *out_u8, int64_t cap) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !w->ready || !w->tex_init) return fail(CSDR_ESTATE, "no textures yet (setup, step, update)");         // :162-164
    if (int rc = wf_check_view(w->fft_size, width, height, mode)) return rc;
    const int64_t pixels = (int64_t)width * height;
    if (out_u8 && cap < 4 * pixels) return fail(CSDR_ERANGE, "need %lld bytes", (long long)(4 * pixels));
    if (int rc = wf_view_tables(w, width, height, mode)) return rc;
    if ((size_t)pixels > w->view.cap) {
        CSDR_HIP_TRY(hipStreamSynchronize(w->st));
        w->view_w = w->view_h = 0;                       // (the buffer csdr_waterfall_device_view handed out goes away)
    }
    if (int rc = w->view.reserve((size_t)pixels)) return rc;
    WfViewArgs a{};
    a.ring[0] = w->ring_of(0); a.ring[1] = w->ring_of(1); a.table = w->table.p;
    a.cols = w->taps.dev.p; a.rows = w->taps.dev.p + width; a.out = w->view.p;
    a.width = width; a.height = height; a.pitch = w->pitch; a.lines = w->lines; a.ofs = w->ofs[0];
    if (mode == CSDR_WF_VIEW_LINEAR) {
        const int groups = (width + 3) / 4;
        const dim3 grid((unsigned)((groups + kWfThreads - 1) / kWfThreads), (unsigned)height);
        WF_LAUNCH(w, KID_WF_VIEW_LINEAR, wf_view_linear, grid, 256 * sizeof(uint32_t), a);
    } else {
        a.n0 = width / 2; a.tile0 = w->peak_tile[0]; a.tile1 = w->peak_tile[1]; a.slots = w->peak_slots;
        a.tiles0 = (a.n0 + a.tile0 - 1) / a.tile0;
        const int tiles1 = (width - a.n0 + a.tile1 - 1) / a.tile1;
        const dim3 grid((unsigned)(a.tiles0 + tiles1), (unsigned)height);
        WF_LAUNCH(w, KID_WF_VIEW_PEAK, wf_view_peak, grid, 256 * sizeof(uint32_t) + (size_t)a.slots * 16, a);
    }
    CSDR_HIP_TRY(hipGetLastError());
    w->view_w = width; w->view_h = height;
    if (out_u8) {
        CSDR_HIP_TRY(hipMemcpyAsync(out_u8, w->view.p, (size_t)(4 * pixels), hipMemcpyDeviceToHost, w->st));
        CSDR_HIP_TRY(hipStreamSynchronize(w->st));
    }
    return CSDR_OK;
}

extern "C" int csdr_waterfall_device_view(csdr_waterfall *w, const uint8_t **dev, int *width, int *height) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !dev) return fail(CSDR_EINVAL, "null argument");
    if (!w->ready || w->view_w == 0) return fail(CSDR_ESTATE, "nothing rendered yet (csdr_waterfall_render_view)");
    if (int rc = w->hand_over()) return rc;
    *dev = reinterpret_cast<const uint8_t *>(w->view.p);
    if (width) *width = w->view_w;
    if (height) *height = w->view_h;
    return CSDR_OK;
}
