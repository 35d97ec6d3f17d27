// overlay_host.hpp -- the compositing rule of csdr_overlay (include/csdr_hip.h, "Overlay bank"), stated once: which pixels a primitive covers, the
// effective alpha under a mask and the three blends.  The kernel (kernels_overlay.hpp) calls these very functions on the device; the object's
// argument checks below are host only.  All integer: every product stays below 2^16 + 2^7.
#pragma once
#include "common.hpp"

namespace csdr {

constexpr int kOvlMaxSide = 16384, kOvlMaxTiles = 1 << 20, kOvlMaxPrims = 1 << 22, kOvlMaxOrigin = 1 << 20;

// csdr_overlay_prim as the kernel reads it: rgba[0..3] is one little-endian word, R in the low byte -- the layout of a pixel of the picture
struct OvlPrim {
    int32_t x, y, w, h;
    uint32_t rgba;
    int32_t mode, mask_x, mask_y;
};
static_assert(sizeof(OvlPrim) == sizeof(csdr_overlay_prim) && offsetof(OvlPrim, rgba) == offsetof(csdr_overlay_prim, rgba) &&
              offsetof(OvlPrim, mask_x) == offsetof(csdr_overlay_prim, mask_x), "OvlPrim is csdr_overlay_prim");

// x <= p < x + w without forming x + w (|x| <= 2^20, p < 2^14: the difference fits; w >= 0)
__host__ __device__ inline bool ovl_inside(int p, int x, int w) { return (uint32_t)(p - x) < (uint32_t)w; }
// does the primitive touch the pixel block [c0, c1) x [r0, r1) of its tile?
__host__ __device__ inline bool ovl_touches(const OvlPrim &q, int c0, int c1, int r0, int r1) {
    return q.w > 0 && q.h > 0 && q.x < c1 && (int64_t)q.x + q.w > c0 && q.y < r1 && (int64_t)q.y + q.h > r0;
}
__host__ __device__ inline uint32_t ovl_div255(uint32_t v) { return (v + 127u) / 255u; }
__host__ __device__ inline uint32_t ovl_masked_alpha(uint32_t a, uint32_t cov) { return ovl_div255(a * cov); }
// where the mask byte of tile pixel (px, py) lies in a plane font_w bytes wide: the window starts at the primitive's unclipped origin
__host__ __device__ inline int64_t ovl_mask_at(const OvlPrim &q, int px, int py, int font_w) {
    return (int64_t)(q.mask_y + (py - q.y)) * font_w + (q.mask_x + (px - q.x));
}
// one pixel d under colour word s (its alpha byte is not read: OVER and ADD take 255 for the A byte) at effective alpha ae
__host__ __device__ inline uint32_t ovl_blend(uint32_t d, uint32_t s, uint32_t ae, int mode) {
    if (mode == CSDR_OVL_COPY) return (s & 0x00ffffffu) | (ae << 24);
    const uint32_t src = s | 0xff000000u;
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 32; ch += 8) {
        const uint32_t sc = (src >> ch) & 0xffu, dc = (d >> ch) & 0xffu;
        uint32_t v;
        if (mode == CSDR_OVL_OVER) v = ovl_div255(sc * ae + dc * (255u - ae));
        else { v = dc + ovl_div255(sc * ae); v = v > 255u ? 255u : v; }
        out |= v << ch;
    }
    return out;
}

// ---- host only: the checks of a compose ----
inline int ovl_check_geometry(int width, int height, int n_tiles, int atlas_cols) {
    if (width < 1 || width > kOvlMaxSide || height < 1 || height > kOvlMaxSide) return fail(CSDR_EINVAL, "a tile of %d x %d (1 .. 16384 each)", width, height);
    if (n_tiles < 1 || atlas_cols < 1 || atlas_cols > n_tiles) return fail(CSDR_EINVAL, "atlas_cols %d: 1 .. n_tiles (%d)", atlas_cols, n_tiles);
    return CSDR_OK;
}
inline int ovl_check_prim(const csdr_overlay_prim &q, int i, int font_w, int font_h) {
    if (q.mode < CSDR_OVL_OVER || q.mode > CSDR_OVL_COPY) return fail(CSDR_EINVAL, "primitive %d: mode %d (0 .. 2)", i, q.mode);
    if (q.w < 0 || q.h < 0) return fail(CSDR_EINVAL, "primitive %d: a size of %d x %d", i, q.w, q.h);
    if (q.x < -kOvlMaxOrigin || q.x > kOvlMaxOrigin || q.y < -kOvlMaxOrigin || q.y > kOvlMaxOrigin) return fail(CSDR_EINVAL, "primitive %d: origin (%d, %d) beyond 2^20", i, q.x, q.y);
    if (q.mask_x >= 0) {
        if (font_w == 0) return fail(CSDR_EINVAL, "primitive %d has a mask and no font is set (csdr_overlay_set_font)", i);
        if (q.mask_y < 0 || (int64_t)q.mask_x + q.w > font_w || (int64_t)q.mask_y + q.h > font_h)
            return fail(CSDR_EINVAL, "primitive %d: its window (%d, %d) + %d x %d leaves the font plane of %d x %d", i, q.mask_x, q.mask_y, q.w, q.h, font_w, font_h);
    }
    return CSDR_OK;
}

}  // namespace csdr
