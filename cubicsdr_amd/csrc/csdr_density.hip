// csdr_density.hip -- implementation of include/csdr_hip.h (gfx950): csdr_density, a bank of hit grids in HBM -- how often the trace passed through
// every pixel of a tile -- stepped with all frames of any number of items and drawn through a palette as tiles of one RGBA8 atlas with the geometry
// of csdr_wfbank_render.  A step checks its items, stages the host ones behind the item records in ONE upload and launches density_cover and
// density_fold once each; a render uploads its views and launches density_render once (kernels_density.hpp).  The rule all three follow is
// density_host.hpp; csdr_design_density_cover is that rule on the host.  All work runs on a stream of the object's own (stream_order.hpp); device
// points are ordered behind the boundary stream by an event, a spectrum's and a spectrum bank's points by their reader gates.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#define CSDR_TU_DENSITY 1  // this unit is the home of its kernels (kernels_density.hpp)
#include "csdr_objects.hpp"
#include "kernels_density.hpp"

using namespace csdr;

static_assert(sizeof(csdr_density_item) == 48 && offsetof(csdr_density_item, slot) == 16 && offsetof(csdr_density_item, weight) == 44, "csdr_density_item layout");

namespace {
constexpr int kDnStage = 2;                              // page-locked staging sets of the records and the staged points
}  // namespace

struct csdr_density : SideStream {                       // (ev_in: device points of the caller; ev_out: csdr_density_device_view)
    bool ready = false;
    int W = 0, H = 0, max_slots = 0, max_frames = 0, max_points = 0;
    int col_blocks = 0, bands = 0, fold_groups = 0, Wp = 0, Hp = 0;
    DevBuf<uint32_t> count, blockmax, palette, planes, view;
    bool palette_set = false;
    int view_w = 0, view_h = 0;                          // in pixels; 0: none
    StageRing<kDnStage> plan;                            // the records of the call being run and the staged host points behind them
    std::vector<char> named;                             // a step's slots
    std::vector<csdr_density_item> sb_items;             // csdr_density_step_specbank's list
    int n_blocks() const { return col_blocks * fold_groups; }
    size_t cells() const { return (size_t)W * (size_t)H; }
};

#define DN_LAUNCH(d_, kid_, kern_, grid_, threads_, lds_, ...) \
    do { ProfScope ps__((d_)->ctx, (kid_), (d_)->st); hipLaunchKernelGGL(kern_, grid_, dim3((unsigned)(threads_)), lds_, (d_)->st, __VA_ARGS__); } while (0)

extern "C" int csdr_design_density_cover(const float *points, int n, int layout, int64_t stride_floats, int frames, int kind, int width, int height, uint32_t *cover) {
    return density_cover_host(points, n, layout, stride_floats, frames, kind, width, height, cover);
}

extern "C" int csdr_density_create(csdr_ctx *ctx, csdr_density **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    std::unique_ptr<csdr_density, void (*)(csdr_density *)> d(new csdr_density(), csdr_density_destroy);
    if (int rc = d->create(ctx)) return rc;
    if (int rc = d->plan.create()) return rc;
    *out = d.release();
    return CSDR_OK;
}

extern "C" void csdr_density_destroy(csdr_density *d) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d) return;
    d->destroy();
    d->plan.destroy();
    d->count.release(); d->blockmax.release(); d->palette.release(); d->planes.release(); d->view.release();
    delete d;
}

static int dn_upload_palette(csdr_density *d, const uint8_t *rgba) {
    uint32_t tab[256];
    for (int i = 0; i < 256; ++i)
        tab[i] = rgba ? (uint32_t)rgba[4 * i] | ((uint32_t)rgba[4 * i + 1] << 8) | ((uint32_t)rgba[4 * i + 2] << 16) | ((uint32_t)rgba[4 * i + 3] << 24)
                      : 0xff000000u | (uint32_t)i * 0x010101u;
    if (int rc = d->palette.reserve(256)) return rc;
    CSDR_HIP_TRY(hipStreamSynchronize(d->st));           // (a render may still read the table; the copy below is from the stack)
    CSDR_HIP_TRY(hipMemcpy(d->palette.p, tab, sizeof tab, hipMemcpyHostToDevice));
    return CSDR_OK;
}

extern "C" int csdr_density_setup(csdr_density *d, int width, int height, int max_slots, int max_frames, int max_points) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d) return fail(CSDR_EINVAL, "density bank is null");
    if (int rc = density_check_tile(width, height)) return rc;
    if (max_slots < 1 || (int64_t)max_slots * width * height > kDnMaxCells) return fail(CSDR_EINVAL, "max_slots %d: 1 .. 2^30 / (width * height)", max_slots);
    if (max_frames < 1 || max_frames > kDnMaxFrames) return fail(CSDR_EINVAL, "max_frames %d: 1 .. 2^20", max_frames);
    if (max_points < 1 || max_points > kTraceMaxPoints) return fail(CSDR_EINVAL, "max_points %d: 1 .. 2^21", max_points);
    CSDR_HIP_TRY(hipStreamSynchronize(d->st));
    d->ready = false;
    d->view_w = d->view_h = 0;
    const int col_blocks = (width + kDnCols - 1) / kDnCols, fold_groups = (height + kDnFoldRows - 1) / kDnFoldRows;
    if (int rc = d->count.reserve((size_t)max_slots * width * height)) return rc;
    if (int rc = d->blockmax.reserve((size_t)max_slots * col_blocks * fold_groups)) return rc;
    if (!d->palette_set || !d->palette.p) if (int rc = dn_upload_palette(d, nullptr)) return rc;
    d->W = width; d->H = height; d->max_slots = max_slots; d->max_frames = max_frames; d->max_points = max_points;
    d->col_blocks = col_blocks; d->fold_groups = fold_groups;
    d->bands = (height + kDnBand - 1) / kDnBand;
    d->Wp = col_blocks * kDnCols; d->Hp = (height + 1) / 2;
    CSDR_HIP_TRY(hipMemsetAsync(d->count.p, 0, (size_t)max_slots * d->cells() * sizeof(uint32_t), d->st));
    CSDR_HIP_TRY(hipMemsetAsync(d->blockmax.p, 0, (size_t)max_slots * d->n_blocks() * sizeof(uint32_t), d->st));
    d->named.assign((size_t)max_slots, 0);
    d->ready = true;
    return CSDR_OK;
}

extern "C" int csdr_density_set_palette(csdr_density *d, const uint8_t *rgba) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !rgba) return fail(CSDR_EINVAL, "null argument");
    if (int rc = dn_upload_palette(d, rgba)) return rc;
    d->palette_set = true;
    return CSDR_OK;
}

extern "C" int csdr_density_reset_slot(csdr_density *d, int slot) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !d->ready) return fail(CSDR_ESTATE, "density bank not set up");
    if (slot < 0 || slot >= d->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, d->max_slots);
    CSDR_HIP_TRY(hipMemsetAsync(d->count.p + (size_t)slot * d->cells(), 0, d->cells() * sizeof(uint32_t), d->st));
    CSDR_HIP_TRY(hipMemsetAsync(d->blockmax.p + (size_t)slot * d->n_blocks(), 0, (size_t)d->n_blocks() * sizeof(uint32_t), d->st));
    return CSDR_OK;
}

// item 6: a refused list changes nothing
static int dn_check_items(csdr_density *d, const csdr_density_item *items, int n_items) {
    if (n_items < 1 || n_items > d->max_slots || !items) return fail(CSDR_EINVAL, "n_items %d: 1 .. max_slots (%d), no null pointer", n_items, d->max_slots);
    std::fill(d->named.begin(), d->named.end(), 0);
    for (int i = 0; i < n_items; ++i) {
        const csdr_density_item &it = items[i];
        if (it.slot < 0 || it.slot >= d->max_slots) return fail(CSDR_EINVAL, "item %d: slot %d of %d", i, it.slot, d->max_slots);
        if (d->named[(size_t)it.slot]) return fail(CSDR_EINVAL, "item %d: slot %d is named twice", i, it.slot);
        d->named[(size_t)it.slot] = 1;
        if (int rc = density_check_frames(it.points, it.n, it.layout, it.stride_floats, it.frames, it.kind)) return rc;
        if (it.is_dev != 0 && it.is_dev != 1) return fail(CSDR_EINVAL, "item %d: is_dev %d", i, it.is_dev);
        if (it.keep_q16 > kDnMaxKeep) return fail(CSDR_EINVAL, "item %d: keep_q16 %u: 0 .. 65536", i, it.keep_q16);
        if (it.weight < 1 || it.weight > kDnMaxWeight) return fail(CSDR_EINVAL, "item %d: weight %u: 1 .. 2^24", i, it.weight);
        if (it.points && it.is_dev && ((uintptr_t)it.points & 3)) return fail(CSDR_EINVAL, "item %d: device points must be 4-byte aligned", i);
    }
    for (int i = 0; i < n_items; ++i) {
        if (items[i].n > d->max_points) return fail(CSDR_ERANGE, "item %d: n %d exceeds max_points %d", i, items[i].n, d->max_points);
        if (items[i].frames > d->max_frames) return fail(CSDR_ERANGE, "item %d: frames %d exceed max_frames %d", i, items[i].frames, d->max_frames);
    }
    return CSDR_OK;
}

// the checked list: records and staged host points in one upload, then the two launches.  `dc`: the DC-spike overwrite of every item's frames
static int dn_step(csdr_density *d, const csdr_density_item *items, int n_items, const HideDcSpan &dc, bool caller_points) {
    size_t host_floats = 0, plane_words = 0;
    int max_chunks = 0;
    bool any_dev = false;
    const size_t plane = (size_t)d->Hp * (size_t)d->Wp;
    for (int i = 0; i < n_items; ++i) {
        const csdr_density_item &it = items[i];
        if (!density_item_reads(it.points, it.n, it.frames)) continue;
        const int chunks = (it.frames + kDnChunk - 1) / kDnChunk;
        max_chunks = std::max(max_chunks, chunks);
        plane_words += (size_t)chunks * plane;
        if (it.is_dev) any_dev = true;
        else host_floats += (size_t)it.frames * (((size_t)it.n * (size_t)(1 + it.layout) + 3) / 4 * 4);
    }
    if (plane_words > d->planes.cap) CSDR_HIP_TRY(hipStreamSynchronize(d->st));           // (a kernel may still read the buffer being replaced)
    if (int rc = d->planes.reserve(plane_words)) return rc;
    const size_t points_at = ((size_t)n_items * sizeof(DnJob) + 15) / 16 * 16, bytes = points_at + host_floats * sizeof(float);
    if (int rc = d->plan.begin(d->st, bytes)) return rc;
    if (any_dev && caller_points) if (int rc = d->after_boundary()) return rc;            // the caller produced them on the boundary stream
    DnJob *jobs = reinterpret_cast<DnJob *>(d->plan.host());
    float *stage_h = reinterpret_cast<float *>(d->plan.host() + points_at);
    const float *stage_d = reinterpret_cast<const float *>(d->plan.device() + points_at);
    size_t at = 0, plane_at = 0;
    for (int i = 0; i < n_items; ++i) {
        const csdr_density_item &it = items[i];
        DnJob jb{};
        jb.slot = it.slot; jb.keep_q16 = it.keep_q16; jb.weight = it.weight; jb.kind = it.kind; jb.stride = 1 + it.layout;
        if (density_item_reads(it.points, it.n, it.frames)) {
            jb.n = it.n; jb.frames = it.frames; jb.dc = dc;
            jb.n_chunks = (it.frames + kDnChunk - 1) / kDnChunk;
            jb.plane0 = (int64_t)plane_at;
            plane_at += (size_t)jb.n_chunks * plane;
            if (it.is_dev) { jb.pts = it.points; jb.frame_stride = it.stride_floats; }
            else {                                       // a staged frame starts on a 16-byte boundary
                const size_t nf = (size_t)it.n * (size_t)(1 + it.layout), pitch = (nf + 3) / 4 * 4;
                for (int f = 0; f < it.frames; ++f) memcpy(stage_h + at + (size_t)f * pitch, it.points + (int64_t)f * it.stride_floats, nf * sizeof(float));
                jb.pts = stage_d + at; jb.frame_stride = (int64_t)pitch;
                at += (size_t)it.frames * pitch;
            }
        }
        jobs[i] = jb;
    }
    if (int rc = d->plan.uploaded(d->st, points_at + at * sizeof(float))) return rc;
    DnArgs a{};
    a.jobs = reinterpret_cast<const DnJob *>(d->plan.device());
    a.planes = d->planes.p; a.count = d->count.p; a.blockmax = d->blockmax.p;
    a.W = d->W; a.H = d->H; a.Wp = d->Wp; a.Hp = d->Hp; a.col_blocks = d->col_blocks; a.bands = d->bands; a.fold_groups = d->fold_groups;
    // (a list of decay-only items still launches density_cover: one row of workgroups that leave at once)
    DN_LAUNCH(d, KID_DENSITY_COVER, density_cover, dim3((unsigned)((size_t)n_items * d->col_blocks * d->bands), (unsigned)std::max(1, max_chunks)), kDnCols,
              dn_cover_lds(d->H), a);
    DN_LAUNCH(d, KID_DENSITY_FOLD, density_fold, dim3((unsigned)((size_t)n_items * d->col_blocks), (unsigned)d->fold_groups), kDnThreads,
              (kDnThreads / 64) * sizeof(uint32_t), a);
    CSDR_HIP_TRY(hipGetLastError());
    return CSDR_OK;
}

extern "C" int csdr_density_step(csdr_density *d, const csdr_density_item *items, int n_items) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !d->ready) return fail(CSDR_ESTATE, "density bank not set up");
    if (int rc = dn_check_items(d, items, n_items)) return rc;
    return dn_step(d, items, n_items, HideDcSpan(), true);
}

extern "C" int csdr_density_step_spec(csdr_density *d, int slot, csdr_spec *spec, int frame0, int n_frames, uint32_t keep_q16, uint32_t weight) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !d->ready) return fail(CSDR_ESTATE, "density bank not set up");
    if (!spec) return fail(CSDR_EINVAL, "spec is null");
    SpecPointsRef ref;
    if (int rc = spec_points_acquire(spec, d->st, &ref)) return rc;
    // (every way out from here passes the release: an acquire is never left unpaired)
    int rc = CSDR_OK;
    if (ref.ctx != d->ctx) rc = fail(CSDR_EINVAL, "the spectrum belongs to another context");
    else if (frame0 < 0 || n_frames < 0 || frame0 + (int64_t)n_frames > ref.frames) rc = fail(CSDR_EINVAL, "frames %d .. %d of %d", frame0, frame0 + n_frames, ref.frames);
    else {
        const csdr_density_item it{n_frames > 0 ? ref.points + (size_t)frame0 * ref.F : nullptr, ref.F, slot, ref.F, n_frames, 0, CSDR_TRACE_SPECTRUM, 1, keep_q16, weight};
        rc = dn_check_items(d, &it, 1);
        if (rc == CSDR_OK) rc = dn_step(d, &it, 1, ref.dc, false);
    }
    if (int r2 = spec_points_release(spec, d->st)) return r2;
    return rc;
}

extern "C" int csdr_density_step_specbank(csdr_density *d, csdr_specbank *sb, uint32_t keep_q16, uint32_t weight) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !d->ready) return fail(CSDR_ESTATE, "density bank not set up");
    if (!sb) return fail(CSDR_EINVAL, "spectrum bank is null");
    SpecBankPointsRef ref;
    if (int rc = specbank_points_acquire(sb, d->st, &ref)) return rc;
    int rc = CSDR_OK;                                    // (every way out from here passes the release)
    if (ref.ctx != d->ctx) rc = fail(CSDR_EINVAL, "the spectrum bank belongs to another context");
    else {
        d->sb_items.clear();
        const int ns = std::min(d->max_slots, ref.max_slots);
        for (int s = 0; s < ns; ++s) {
            const int f = std::max(0, csdr_specbank_frames(sb, s));
            d->sb_items.push_back(csdr_density_item{f > 0 ? ref.points + (size_t)s * (size_t)ref.max_frames * (size_t)ref.F : nullptr, ref.F, s, ref.F, f, 0,
                                                    CSDR_TRACE_SPECTRUM, 1, keep_q16, weight});
        }
        rc = dn_check_items(d, d->sb_items.data(), (int)d->sb_items.size());
        if (rc == CSDR_OK) rc = dn_step(d, d->sb_items.data(), (int)d->sb_items.size(), HideDcSpan(), false);
    }
    if (int r2 = specbank_points_release(sb, d->st)) return r2;
    return rc;
}

extern "C" int csdr_density_peak(csdr_density *d, int slot, uint32_t *peak) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !d->ready) return fail(CSDR_ESTATE, "density bank not set up");
    if (!peak) return fail(CSDR_EINVAL, "null argument");
    if (slot < 0 || slot >= d->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, d->max_slots);
    std::vector<uint32_t> mx((size_t)d->n_blocks());
    CSDR_HIP_TRY(hipMemcpyAsync(mx.data(), d->blockmax.p + (size_t)slot * d->n_blocks(), mx.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, d->st));
    CSDR_HIP_TRY(hipStreamSynchronize(d->st));
    *peak = *std::max_element(mx.begin(), mx.end());
    return CSDR_OK;
}

extern "C" int csdr_density_fetch(csdr_density *d, int slot, uint32_t *out, int64_t cap) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !d->ready) return fail(CSDR_ESTATE, "density bank not set up");
    if (!out) return fail(CSDR_EINVAL, "null argument");
    if (slot < 0 || slot >= d->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, d->max_slots);
    if (cap < (int64_t)d->cells()) return fail(CSDR_ERANGE, "need %lld entries", (long long)d->cells());
    CSDR_HIP_TRY(hipMemcpyAsync(out, d->count.p + (size_t)slot * d->cells(), d->cells() * sizeof(uint32_t), hipMemcpyDeviceToHost, d->st));
    CSDR_HIP_TRY(hipStreamSynchronize(d->st));
    return CSDR_OK;
}

extern "C" int csdr_density_render(csdr_density *d, const csdr_density_view *views, int n_views, int atlas_cols, uint8_t *out_u8, int64_t cap) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !d->ready) return fail(CSDR_ESTATE, "density bank not set up");
    if (n_views < 1 || n_views > kDnMaxViews || !views) return fail(CSDR_EINVAL, "n_views %d: 1 .. 2^20, no null pointer", n_views);
    if (atlas_cols < 1 || atlas_cols > n_views) return fail(CSDR_EINVAL, "atlas_cols %d: 1 .. n_views (%d)", atlas_cols, n_views);
    for (int k = 0; k < n_views; ++k)
        if (views[k].slot < -1 || views[k].slot >= d->max_slots) return fail(CSDR_EINVAL, "view %d: slot %d of %d", k, views[k].slot, d->max_slots);
    const int tile_rows = (n_views + atlas_cols - 1) / atlas_cols;
    const int64_t n_tiles = (int64_t)tile_rows * atlas_cols;
    const int64_t pic_w = (int64_t)atlas_cols * d->W, pic_h = (int64_t)tile_rows * d->H, pixels = pic_w * pic_h;
    if (pic_w > 0x7fffffff || pic_h > 0x7fffffff || n_tiles * d->col_blocks > 0x7fffffff) return fail(CSDR_EINVAL, "an atlas of %lld x %lld pixels", (long long)pic_w, (long long)pic_h);
    if (out_u8 && cap < 4 * pixels) return fail(CSDR_ERANGE, "need %lld bytes", (long long)(4 * pixels));
    // ---- from here on only the device can refuse
    if ((size_t)pixels > d->view.cap) {
        CSDR_HIP_TRY(hipStreamSynchronize(d->st));
        d->view_w = d->view_h = 0;                       // (the buffer csdr_density_device_view handed out goes away)
    }
    if (int rc = d->view.reserve((size_t)pixels)) return rc;
    const size_t bytes = (size_t)n_tiles * sizeof(csdr_density_view);
    if (int rc = d->plan.begin(d->st, bytes)) return rc;
    csdr_density_view *vh = reinterpret_cast<csdr_density_view *>(d->plan.host());
    for (int64_t k = 0; k < n_tiles; ++k) vh[k] = k < n_views ? views[k] : csdr_density_view{-1, 0u};
    if (int rc = d->plan.uploaded(d->st, bytes)) return rc;
    DnRenderArgs a{};
    a.views = reinterpret_cast<const csdr_density_view *>(d->plan.device());
    a.count = d->count.p; a.blockmax = d->blockmax.p; a.palette = d->palette.p; a.out = d->view.p;
    a.W = d->W; a.H = d->H; a.atlas_cols = atlas_cols; a.col_blocks = d->col_blocks; a.n_blocks = d->n_blocks();
    DN_LAUNCH(d, KID_DENSITY_RENDER, density_render, dim3((unsigned)(n_tiles * d->col_blocks), (unsigned)((d->H + kDnRenderRows - 1) / kDnRenderRows)), kDnThreads,
              (256 + kDnThreads / 64) * sizeof(uint32_t), a);
    CSDR_HIP_TRY(hipGetLastError());
    d->view_w = (int)pic_w; d->view_h = (int)pic_h;
    if (out_u8) {
        CSDR_HIP_TRY(hipMemcpyAsync(out_u8, d->view.p, (size_t)(4 * pixels), hipMemcpyDeviceToHost, d->st));
        CSDR_HIP_TRY(hipStreamSynchronize(d->st));
    }
    return CSDR_OK;
}

extern "C" int csdr_density_device_view(csdr_density *d, const uint8_t **dev, int *pic_width, int *pic_height) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !dev) return fail(CSDR_EINVAL, "null argument");
    if (!d->ready || d->view_w == 0) return fail(CSDR_ESTATE, "nothing rendered yet (csdr_density_render)");
    if (int rc = d->hand_over()) return rc;
    *dev = reinterpret_cast<const uint8_t *>(d->view.p);
    if (pic_width) *pic_width = d->view_w;
    if (pic_height) *pic_height = d->view_h;
    return CSDR_OK;
}
