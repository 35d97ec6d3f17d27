// kernels_overlay.hpp -- the overlay bank (gfx950): ordered lists of rectangles and glyph windows composited onto the tiles of one RGBA8 atlas.
//
//   dB grid                                    src/panel/SpectrumPanel.cpp:117-147             CSDR_OVL_ADD rows
//   frequency ticks, MHz and dB labels         src/panel/SpectrumPanel.cpp:171-303             rectangles, masked rectangles (glyphs)
//   demodulator markers and labels             src/visual/PrimaryGLContext.cpp:65-199          CSDR_OVL_OVER / _ADD rectangles, glyphs
//
// The picture is the library's own definition (include/csdr_hip.h, "Overlay bank"); its arithmetic is stated once in overlay_host.hpp and called
// from here.  ONE launch composites every tile.  A pixel is owned by one work-item, which applies the tile's list to it in order: exact paint order
// with no atomics and no scratch.
// Home unit: csdr_overlay.hip.
#pragma once
#include "common.hpp"
#include "kernels_waterfall.hpp"
#include "overlay_host.hpp"

#if defined(CSDR_TU_OVERLAY)
#define CSDR_KERNEL_OVL CSDR_KERNEL
#else
#define CSDR_KERNEL_OVL CSDR_KERNEL_ELSEWHERE
#endif

namespace csdr {

constexpr int kOvThreads = 256, kOvWaves = kOvThreads / 64;
constexpr int kOvCols = 64;                  // columns of a tile to a workgroup: 256 bytes of every picture row
constexpr int kOvRows = kOvThreads / (kOvCols / 4);      // picture rows a workgroup covers per row group: 16 work-items of 4 pixels to a row
constexpr int kOvGroups = 4;                 // row groups a work-item may own: its pixels stay in 4 x 4 registers through the whole list
constexpr int kOvChunk = kOvThreads;         // primitives of a list looked at per pass, one to a work-item: 8 KiB of LDS for the survivors
constexpr size_t kOvLds = (size_t)kOvChunk * sizeof(OvlPrim) + kOvWaves * sizeof(int);

struct OvlArgs {
    const csdr_overlay_tile *tiles;          // [n_tiles]
    const OvlPrim *prims;                    // the call's primitives, 16-byte aligned
    const uint32_t *base;                    // the base picture, or nullptr: zero bytes
    uint32_t *out;                           // [tile rows * height][atlas_cols * width] pixels, dense, 16-byte aligned
    const uint8_t *font;                     // [font_h][font_w] coverage bytes
    int font_w;
    int n_tiles;                             // tiles in use; the grid also covers the unused ones of the last tile row
    int width, height, atlas_cols;
    int col_blocks;                          // workgroups along a tile row
    int groups;                              // row groups to a workgroup, 1 .. kOvGroups: it covers kOvRows * groups rows
    int base_vec;                            // `base` is 16-byte aligned: whole groups of 4 pixels are loaded at once
};

__device__ __forceinline__ int64_t ovl_pixel(const OvlArgs &a, int tile, int row, int px) {
    return ((int64_t)(tile / a.atlas_cols) * a.height + row) * ((int64_t)a.atlas_cols * a.width) + (int64_t)(tile % a.atlas_cols) * a.width + px;
}

// grid (all tiles * col_blocks, blocks of kOvRows * groups rows).  A work-item owns 4 neighbouring pixels of one row in each of its row groups: one
// 16-byte load of the base and one 16-byte store each (pixel by pixel where the width or the atlas stride leaves the address off the 16-byte grid,
// as wf_store4 does).  The tile's list comes through LDS kOvChunk primitives at a time: every work-item reads one, tests it against the workgroup's
// pixel block, and the survivors are written to LDS IN LIST ORDER -- an inclusive prefix sum of the keep flags by __shfl_up within each wave, the
// waves' totals through LDS -- so a workgroup walks only what touches its block, every lane reading the same LDS address.  Three barriers per chunk.
CSDR_KERNEL_OVL __launch_bounds__(kOvThreads) void overlay_compose(OvlArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    OvlPrim *kept = reinterpret_cast<OvlPrim *>(smem);                           // [kOvChunk]
    int *wave_n = reinterpret_cast<int *>(smem + (size_t)kOvChunk * sizeof(OvlPrim));    // [kOvWaves]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = (int)(blockIdx.x / (unsigned)a.col_blocks);
    const int c0 = (int)(blockIdx.x % (unsigned)a.col_blocks) * kOvCols, c1 = min(a.width, c0 + kOvCols);
    const int r0 = (int)blockIdx.y * kOvRows * a.groups, r1 = min(a.height, r0 + kOvRows * a.groups);
    const int px0 = c0 + 4 * (tid & (kOvCols / 4 - 1)), cnt = max(0, min(4, a.width - px0)), row0 = r0 + tid / (kOvCols / 4);
    const bool used = tile < a.n_tiles;
    int first = 0, count = 0;
    if (used) { const csdr_overlay_tile tl = a.tiles[tile]; first = tl.first; count = tl.count; }

    uint32_t d[kOvGroups][4];
#pragma unroll
    for (int g = 0; g < kOvGroups; ++g) {
        const int r = row0 + g * kOvRows;
#pragma unroll
        for (int k = 0; k < 4; ++k) d[g][k] = 0u;
        if (!used || !a.base || g >= a.groups || r >= r1 || cnt == 0) continue;
        const int64_t at = ovl_pixel(a, tile, r, px0);
        if (a.base_vec && cnt == 4 && (at & 3) == 0) {
            const int4 v = *reinterpret_cast<const int4 *>(a.base + at);
            d[g][0] = (uint32_t)v.x; d[g][1] = (uint32_t)v.y; d[g][2] = (uint32_t)v.z; d[g][3] = (uint32_t)v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < cnt) d[g][k] = a.base[at + k];
        }
    }

    for (int done = 0; done < count; done += kOvChunk) {
        const int i = done + tid;
        OvlPrim q{};
        int keep = 0;
        if (i < count) {
            const int4 *src = reinterpret_cast<const int4 *>(a.prims + ((int64_t)first + i));
            const int4 lo = src[0], hi = src[1];
            q.x = lo.x; q.y = lo.y; q.w = lo.z; q.h = lo.w; q.rgba = (uint32_t)hi.x; q.mode = hi.y; q.mask_x = hi.z; q.mask_y = hi.w;
            keep = ovl_touches(q, c0, c1, r0, r1) ? 1 : 0;
        }
        int incl = keep;                                 // survivors of this wave up to and including this lane
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, (unsigned)o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wave_n[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kOvWaves; ++w) { const int n = wave_n[w]; before += w < wave ? n : 0; total += n; }
        if (keep) kept[before + incl - 1] = q;
        __syncthreads();
        for (int j = 0; j < total; ++j) {
            const OvlPrim p = kept[j];
            const uint32_t alpha = p.rgba >> 24;
#pragma unroll
            for (int g = 0; g < kOvGroups; ++g) {
                const int r = row0 + g * kOvRows;
                if (g >= a.groups || r >= r1 || !ovl_inside(r, p.y, p.h)) continue;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k >= cnt || !ovl_inside(px0 + k, p.x, p.w)) continue;
                    const uint32_t ae = p.mask_x < 0 ? alpha : ovl_masked_alpha(alpha, a.font[ovl_mask_at(p, px0 + k, r, a.font_w)]);
                    d[g][k] = ovl_blend(d[g][k], p.rgba, ae, p.mode);
                }
            }
        }
        __syncthreads();                                 // `kept` and `wave_n` are rewritten by the next chunk
    }

#pragma unroll
    for (int g = 0; g < kOvGroups; ++g) {
        const int r = row0 + g * kOvRows;
        if (g >= a.groups || r >= r1 || cnt == 0) continue;
        wf_store4(a.out, ovl_pixel(a, tile, r, px0), cnt, d[g][0], d[g][1], d[g][2], d[g][3]);
    }
}

}  // namespace csdr
