// csdr_overlay.hip -- implementation of include/csdr_hip.h (gfx950): csdr_overlay, ordered primitive lists -- the dB grid, the frequency ticks, the
// demodulator markers, the glyphs of the labels -- composited onto the tiles of one RGBA8 atlas with the geometry of csdr_wfbank_render.  The object
// holds a font plane and no other state: a compose checks the whole call, stages the tile runs, the primitives and a host base in ONE upload, and
// launches overlay_compose once (kernels_overlay.hpp).  The rule is overlay_host.hpp.  All work runs on a stream of the object's own
// (stream_order.hpp); a device base is ordered behind the boundary stream by an event.  The planners that make such lists (csdr_design_freq_scale,
// _db_grid, _db_labels, _demod_marker, _text) are design.hpp's; their C entry points are design_overlay_capi.hpp, exported from here too.
#include <algorithm>
#include <cstring>
#include <memory>

#define CSDR_TU_OVERLAY 1  // this unit is the home of its kernel (kernels_overlay.hpp)
#include "csdr_objects.hpp"
#include "design_overlay_capi.hpp"
#include "kernels_overlay.hpp"

using namespace csdr;

namespace {
constexpr int kOvStage = 2;                              // page-locked staging sets of the runs, the primitives and a host base
size_t round16(size_t n) { return (n + 15) / 16 * 16; }
}  // namespace

struct csdr_overlay : SideStream {                       // (ev_in: a device base of the caller; ev_out: csdr_overlay_device_view)
    bool ready = false;
    int max_tiles = 0, max_prims = 0;
    DevBuf<uint8_t> font;                                // the coverage plane
    int font_w = 0, font_h = 0;                          // 0: no font
    DevBuf<uint32_t> view;                               // the last composed atlas
    int view_w = 0, view_h = 0;                          // in pixels; 0: none
    StageRing<kOvStage> plan;
};

extern "C" int csdr_overlay_create(csdr_ctx *ctx, csdr_overlay **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    std::unique_ptr<csdr_overlay, void (*)(csdr_overlay *)> ov(new csdr_overlay(), csdr_overlay_destroy);
    if (int rc = ov->create(ctx)) return rc;
    if (int rc = ov->plan.create()) return rc;
    *out = ov.release();
    return CSDR_OK;
}

extern "C" void csdr_overlay_destroy(csdr_overlay *ov) {
    DeviceScope dev__(ov ? ov->ctx : nullptr);
    if (!ov) return;
    ov->destroy();
    ov->plan.destroy();
    ov->view.release();
    ov->font.release();
    delete ov;
}

extern "C" int csdr_overlay_setup(csdr_overlay *ov, int max_tiles, int max_prims) {
    DeviceScope dev__(ov ? ov->ctx : nullptr);
    if (!ov) return fail(CSDR_EINVAL, "overlay is null");
    if (max_tiles < 1 || max_tiles > kOvlMaxTiles) return fail(CSDR_EINVAL, "max_tiles %d: 1 .. 2^20", max_tiles);
    if (max_prims < 1 || max_prims > kOvlMaxPrims) return fail(CSDR_EINVAL, "max_prims %d: 1 .. 2^22", max_prims);
    CSDR_HIP_TRY(hipStreamSynchronize(ov->st));
    ov->max_tiles = max_tiles; ov->max_prims = max_prims;
    ov->view_w = ov->view_h = 0;
    ov->ready = true;
    return CSDR_OK;
}

extern "C" int csdr_overlay_set_font(csdr_overlay *ov, const uint8_t *a8, int font_w, int font_h) {
    DeviceScope dev__(ov ? ov->ctx : nullptr);
    if (!ov) return fail(CSDR_EINVAL, "overlay is null");
    if (a8 && (font_w < 1 || font_w > kOvlMaxSide || font_h < 1 || font_h > kOvlMaxSide)) return fail(CSDR_EINVAL, "a font plane of %d x %d (1 .. 16384 each)", font_w, font_h);
    CSDR_HIP_TRY(hipStreamSynchronize(ov->st));          // a compose may still read the plane being replaced
    ov->font_w = ov->font_h = 0;                         // (no font until the new plane has arrived)
    if (!a8) return CSDR_OK;
    const size_t bytes = (size_t)font_w * (size_t)font_h;
    if (int rc = ov->font.reserve(bytes)) return rc;
    CSDR_HIP_TRY(hipMemcpy(ov->font.p, a8, bytes, hipMemcpyHostToDevice));
    ov->font_w = font_w; ov->font_h = font_h;
    return CSDR_OK;
}

extern "C" int csdr_overlay_compose(csdr_overlay *ov, const uint8_t *base, int base_is_dev, const csdr_overlay_tile *tiles, int n_tiles,
                                    const csdr_overlay_prim *prims, int n_prims, int width, int height, int atlas_cols, uint8_t *out_u8, int64_t cap) {
    DeviceScope dev__(ov ? ov->ctx : nullptr);
    if (!ov || !ov->ready) return fail(CSDR_ESTATE, "overlay not set up");
    // ---- check: a refused call enqueues nothing and changes nothing
    if (int rc = ovl_check_geometry(width, height, n_tiles, atlas_cols)) return rc;
    if (n_tiles > ov->max_tiles) return fail(CSDR_ERANGE, "n_tiles %d exceeds max_tiles %d", n_tiles, ov->max_tiles);
    if (n_prims < 0 || !tiles || (n_prims > 0 && !prims)) return fail(CSDR_EINVAL, "n_prims %d, or a null pointer", n_prims);
    if (n_prims > ov->max_prims) return fail(CSDR_ERANGE, "n_prims %d exceeds max_prims %d", n_prims, ov->max_prims);
    for (int k = 0; k < n_tiles; ++k)
        if (tiles[k].first < 0 || tiles[k].count < 0 || (int64_t)tiles[k].first + tiles[k].count > n_prims)
            return fail(CSDR_EINVAL, "tile %d: its run [%d, %d + %d) leaves the %d primitives", k, tiles[k].first, tiles[k].first, tiles[k].count, n_prims);
    for (int i = 0; i < n_prims; ++i) if (int rc = ovl_check_prim(prims[i], i, ov->font_w, ov->font_h)) return rc;
    if (base && base_is_dev && ((uintptr_t)base & 3)) return fail(CSDR_EINVAL, "a device base must be 4-byte aligned");
    const int tile_rows = (n_tiles + atlas_cols - 1) / atlas_cols;
    const int64_t n_all = (int64_t)tile_rows * atlas_cols;
    const int64_t pic_w = (int64_t)atlas_cols * width, pic_h = (int64_t)tile_rows * height, pixels = pic_w * pic_h;
    const int col_blocks = (width + kOvCols - 1) / kOvCols;
    if (pic_w > 0x7fffffff || pic_h > 0x7fffffff || n_all * col_blocks > 0x7fffffff) return fail(CSDR_EINVAL, "an atlas of %lld x %lld pixels", (long long)pic_w, (long long)pic_h);
    if (out_u8 && cap < 4 * pixels) return fail(CSDR_ERANGE, "need %lld bytes", (long long)(4 * pixels));
    // ---- from here on only the device can refuse
    if ((size_t)pixels > ov->view.cap) {
        CSDR_HIP_TRY(hipStreamSynchronize(ov->st));
        ov->view_w = ov->view_h = 0;                     // (the buffer csdr_overlay_device_view handed out goes away)
    }
    if (int rc = ov->view.reserve((size_t)pixels)) return rc;
    const bool host_base = base && !base_is_dev;
    const size_t prims_at = round16((size_t)n_tiles * sizeof(csdr_overlay_tile)), base_at = prims_at + (size_t)n_prims * sizeof(csdr_overlay_prim);
    const size_t bytes = base_at + (host_base ? (size_t)pixels * 4 : 0);
    if (int rc = ov->plan.begin(ov->st, bytes)) return rc;
    if (base && base_is_dev) if (int rc = ov->after_boundary()) return rc;       // the caller produced it on, or handed it to, the boundary stream
    memcpy(ov->plan.host(), tiles, (size_t)n_tiles * sizeof(csdr_overlay_tile));
    if (n_prims) memcpy(ov->plan.host() + prims_at, prims, (size_t)n_prims * sizeof(csdr_overlay_prim));
    if (host_base) memcpy(ov->plan.host() + base_at, base, (size_t)pixels * 4);
    if (int rc = ov->plan.uploaded(ov->st, bytes)) return rc;
    OvlArgs a{};
    a.tiles = reinterpret_cast<const csdr_overlay_tile *>(ov->plan.device());
    a.prims = reinterpret_cast<const OvlPrim *>(ov->plan.device() + prims_at);
    a.base = !base ? nullptr : reinterpret_cast<const uint32_t *>(host_base ? reinterpret_cast<const uint8_t *>(ov->plan.device() + base_at) : base);
    a.base_vec = ((uintptr_t)a.base & 15) == 0;
    a.out = ov->view.p; a.font = ov->font.p; a.font_w = ov->font_w;
    a.n_tiles = n_tiles; a.width = width; a.height = height; a.atlas_cols = atlas_cols; a.col_blocks = col_blocks;
    // a work-item takes up to kOvGroups row groups: each workgroup reads its tile's whole list once, so the fewer workgroups to a tile the better
    a.groups = std::min(kOvGroups, (height + kOvRows - 1) / kOvRows);
    const dim3 grid((unsigned)(n_all * col_blocks), (unsigned)((height + kOvRows * a.groups - 1) / (kOvRows * a.groups)));
    {
        ProfScope ps__(ov->ctx, KID_OVERLAY_COMPOSE, ov->st);
        hipLaunchKernelGGL(overlay_compose, grid, dim3((unsigned)kOvThreads), kOvLds, ov->st, a);
    }
    CSDR_HIP_TRY(hipGetLastError());
    ov->view_w = (int)pic_w; ov->view_h = (int)pic_h;
    if (out_u8) {
        CSDR_HIP_TRY(hipMemcpyAsync(out_u8, ov->view.p, (size_t)(4 * pixels), hipMemcpyDeviceToHost, ov->st));
        CSDR_HIP_TRY(hipStreamSynchronize(ov->st));
    }
    return CSDR_OK;
}

extern "C" int csdr_overlay_device_view(csdr_overlay *ov, const uint8_t **dev, int *pic_width, int *pic_height) {
    DeviceScope dev__(ov ? ov->ctx : nullptr);
    if (!ov || !dev) return fail(CSDR_EINVAL, "null argument");
    if (!ov->ready || ov->view_w == 0) return fail(CSDR_ESTATE, "nothing composed yet (csdr_overlay_compose)");
    if (int rc = ov->hand_over()) return rc;
    *dev = reinterpret_cast<const uint8_t *>(ov->view.p);
    if (pic_width) *pic_width = ov->view_w;
    if (pic_height) *pic_height = ov->view_h;
    return CSDR_OK;
}
