// kernels_wfbank.hpp -- the waterfall bank (gfx950): N WaterfallPanels of one fft_size and one `lines`, every slot of a call in ONE launch.
//
//   quantise the lines of all slots             src/panel/WaterfallPanel.cpp:39-49, :64-72    wfb_quantize (one job per line, from the host's plan)
//   write every slot's surviving runs           src/panel/WaterfallPanel.cpp:132-158          wfb_update   (two runs per slot, by record)
//   the slots' rings as one atlas of W x H      src/panel/WaterfallPanel.cpp:117-120,         wfb_view_linear (the reference's picture per tile)
//     tiles                                     :161-219                                      wfb_view_peak   (the library's own: max over the footprint)
//
// Every kernel body here is that of kernels_waterfall.hpp and is stated there once: wf_quantize_chunk, wf_stage_table, wf_linear4,
// wf_store4, wf_footprint_max and wf_scan_max are called from here, as they are from the single panel's kernels.  What a kernel of this file keeps
// is where a work-item finds its slot: in a record the host uploads with the call (csdr_wfbank.hip does all integer bookkeeping), so
// the grid covers all slots at once.  Pending rows and ring rows keep the 16-byte pitch; a slot's pending block is max_pending * pitch bytes per
// half and its ring block lines * pitch, both multiples of 16, so every row of every slot starts on a 16-byte boundary.
// Home unit: csdr_wfbank.hip.
#pragma once
#include "common.hpp"
#include "kernels_waterfall.hpp"

#if defined(CSDR_TU_WFBANK)
#define CSDR_KERNEL_WFB CSDR_KERNEL
#else
#define CSDR_KERNEL_WFB CSDR_KERNEL_ELSEWHERE
#endif

namespace csdr {

// One line of one slot.  The host resolves where a line's values lie: a line of the call (the caller's device memory or the staged copy of a host
// line), or -- for a line of the wrong length that repeats the slot's points (WaterfallCanvas.cpp:106-109) -- the good line in front of it in the same
// call, or the slot's kept points from before the call.  So no job reads what another job of the launch writes, and the jobs run in any order:
// the kept points have two copies per slot, a call writes the one the slot does not read from.
enum : int32_t { kWfbPair = 1, kWfbWide = 2 };
struct WfbJob {
    const float *src;          // point p: src[pair ? 2 p + 1 : p]
    float *keep;               // the slot's `points` (:39-49) receive this line's values: the slot's last good line of the call; nullptr: none
    int32_t slot;
    int32_t row;               // pending row of the slot; -1: a dropped step (:60-62), only `keep` is written
    int32_t flags;             // kWfbPair: (x, y) pairs, the y is used; kWfbWide: 16-byte loads are possible (half % 16 == 0, src 16-byte aligned)
    int32_t pad;
};
static_assert(sizeof(WfbJob) == 32, "WfbJob layout");

struct WfbQuantArgs {
    const WfbJob *jobs;
    int n_jobs, half, pitch;
    uint8_t *pend;             // [slot][2 halves][max_pending][pitch]
    int64_t pend_half;         // bytes of one half's pending rows: max_pending * pitch
};

// grid (chunks of a half / block, jobs, 2 halves); the block is as many waves as a half has 16-point chunks (half <= 2048: at most 128 of them)
CSDR_KERNEL_WFB __launch_bounds__(kWfThreads) void wfb_quantize(WfbQuantArgs a) {
    const int j = (int)blockIdx.z;
    const int i0 = ((int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x) * kWfChunk;
    if (i0 >= a.half) return;
    const int cnt = min(kWfChunk, a.half - i0);
    const int p0 = j * a.half + i0;                                   // byte i of half j comes from point j * half + i (:65-67)
    for (int q = (int)blockIdx.y; q < a.n_jobs; q += (int)gridDim.y) {
        const WfbJob jb = a.jobs[q];
        const bool wide = (jb.flags & kWfbWide) != 0 && cnt == kWfChunk;
        wf_quantize_chunk(jb.src, (jb.flags & kWfbPair) != 0, HideDcSpan(), p0, cnt, wide, wide,
                          jb.row >= 0, a.pend + ((int64_t)jb.slot * 2 + j) * a.pend_half + (int64_t)jb.row * a.pitch + i0, jb.keep);       // (the row is 16-byte aligned: every term is)
    }
}

// WaterfallPanel::update (:139-158) of one slot, reduced by the host to the runs whose rows survive (WfRun, kernels_waterfall.hpp)
struct WfbUpdate {
    int32_t slot, n_runs, n_pending, pad;
    WfRun run[2];              // in the order the reference writes them (run[1] last)
};
static_assert(sizeof(WfbUpdate) == 40, "WfbUpdate layout");

struct WfbUpdateArgs {
    const WfbUpdate *upd;      // [slots that have pending lines]
    int pitch;
    uint8_t *ring;             // [slot][2 halves][lines][pitch]
    const uint8_t *pend;       // [slot][2 halves][max_pending][pitch]
    int64_t ring_half, pend_half;
};

// grid (16-byte chunks of a row / block, rows of the longest slot, records x 2 halves)
CSDR_KERNEL_WFB __launch_bounds__(kWfThreads) void wfb_update(WfbUpdateArgs a) {
    const WfbUpdate u = a.upd[blockIdx.z >> 1];
    const int j = (int)(blockIdx.z & 1u);
    const int total = u.run[0].n + (u.n_runs > 1 ? u.run[1].n : 0);
    const int chunks = a.pitch / 16;
    const uint8_t *pend = a.pend + ((int64_t)u.slot * 2 + j) * a.pend_half;
    uint8_t *ring = a.ring + ((int64_t)u.slot * 2 + j) * a.ring_half;
    for (int y = (int)blockIdx.y; y < total; y += (int)gridDim.y) {
        const int r = y < u.run[0].n ? 0 : 1, t = r ? y - u.run[0].n : y;
        const int dst = u.run[r].dst + t;
        // wf_update's rule: a row of the earlier run that the later run writes too is not written at all
        if (r == 0 && u.n_runs > 1 && dst >= u.run[1].dst && dst < u.run[1].dst + u.run[1].n) continue;
        const int4 *s = reinterpret_cast<const int4 *>(pend + (int64_t)(u.n_pending - 1 - u.run[r].src - t) * a.pitch);
        int4 *d = reinterpret_cast<int4 *>(ring + (int64_t)dst * a.pitch);
        for (int c = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x; c < chunks; c += (int)gridDim.x * (int)blockDim.x) d[c] = s[c];
    }
}

// ---- the atlas: tile k of the picture is list entry k's slot, rendered as wf_view_linear / wf_view_peak render one waterfall ----
struct WfbTile {
    int32_t slot;
    int32_t ofs;               // the slot's waterfall_ofs; -1: no textures (or an unused tile of the last tile row) -- all-zero bytes
};
struct WfbViewArgs {
    const WfbTile *tiles;      // [tile rows * atlas_cols]
    const uint8_t *ring;       // [slot][2 halves][lines][pitch]
    int64_t ring_half;
    const uint32_t *table;     // 256 x RGBA8, 16-byte aligned
    const csdr_view_tap *cols, *rows;        // [width], [height]: one table each for all slots (the taps do not depend on the offset)
    uint32_t *out;             // [tile rows * height][atlas_cols * width] pixels, dense
    int width, height, pitch, lines, atlas_cols;
    int groups, per_tile;      // wfb_view_linear: groups of 4 pixels in a tile row; workgroups per tile
    int n0, rows_per, chunks;  // wfb_view_peak: pixels of half 0; image rows per workgroup; 16-byte chunks of a ring row
};

// grid (tiles x workgroups per tile).  A work-item owns 4 consecutive pixels of one image row of one tile; the work-items of a tile are numbered
// row by row, so a workgroup takes 256 / groups image rows of a thumbnail and none of it idles (a 64-pixel row is 16 work-items).
CSDR_KERNEL_WFB __launch_bounds__(kWfThreads) void wfb_view_linear(WfbViewArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t *tab = wf_stage_table(smem, a.table);
    __syncthreads();
    const int tile = (int)(blockIdx.x / (unsigned)a.per_tile);
    const int item = (int)(blockIdx.x % (unsigned)a.per_tile) * kWfThreads + (int)threadIdx.x;
    const int py = item / a.groups, px0 = 4 * (item % a.groups);
    if (py >= a.height) return;
    const int cnt = min(4, a.width - px0);
    const WfbTile tl = a.tiles[tile];
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    if (tl.ofs >= 0) {
        const uint8_t *ring0 = a.ring + (int64_t)tl.slot * 2 * a.ring_half;
        csdr_view_tap ct[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) ct[k] = a.cols[min(px0 + k, a.width - 1)];
        wf_linear4(tab, ring0, ring0 + a.ring_half, a.pitch, a.lines, tl.ofs, ct, a.rows[py], c);
    }
    const int64_t pic_w = (int64_t)a.atlas_cols * a.width;
    // the ATLAS address decides: a tile whose width is no multiple of 4 leaves the tile columns beside it off the 16-byte grid
    wf_store4(a.out, ((int64_t)(tile / a.atlas_cols) * a.height + py) * pic_w + (int64_t)(tile % a.atlas_cols) * a.width + px0, cnt, c[0], c[1], c[2], c[3]);
}

// grid (tiles, groups of rows_per image rows, 2 halves).  A workgroup owns rows_per image rows of one half of one tile.  Pass 1: for each of its
// image rows the element-wise max of the footprint's ring rows over the WHOLE half row, in 16-byte loads, into LDS.  One barrier.  Pass 2: each
// work-item scans its pixels' bytes in LDS word by word and looks the colour of the largest up.  With half <= 2048 a half row is at most 128
// chunks (2 KB), so a row's span always fits and the folded path of wf_view_peak (a pixel wider than the LDS slots) is not needed; taking the
// whole row instead of the pixels' span costs nothing either, every pixel of the half lies in this workgroup.  The padding of a ring row is
// zero and no pixel's bytes reach into it.
CSDR_KERNEL_WFB __launch_bounds__(kWfThreads) void wfb_view_peak(WfbViewArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t *tab = wf_stage_table(smem, a.table);
    int4 *span = reinterpret_cast<int4 *>(smem + 256 * sizeof(uint32_t));      // [rows_per][chunks]
    const int tid = (int)threadIdx.x;
    const int tile = (int)blockIdx.x, h = (int)blockIdx.z;
    const int py0 = (int)blockIdx.y * a.rows_per, nr = min(a.rows_per, a.height - py0);
    const WfbTile tl = a.tiles[tile];
    if (tl.ofs >= 0) {
        const uint8_t *ring = a.ring + ((int64_t)tl.slot * 2 + h) * a.ring_half;
        for (int s = tid; s < nr * a.chunks; s += kWfThreads) {
            const int r = s / a.chunks, cc = s - r * a.chunks;
            const csdr_view_tap rt = a.rows[py0 + r];
            span[s] = wf_footprint_max(ring + 16 * (int64_t)cc, a.pitch, a.lines, (int)(((int64_t)tl.ofs + rt.first) % a.lines), rt.count);
        }
    }
    __syncthreads();
    const int nh = h ? a.width - a.n0 : a.n0, x0 = h ? a.n0 : 0;
    const int64_t pic_w = (int64_t)a.atlas_cols * a.width;
    uint32_t *out = a.out + ((int64_t)(tile / a.atlas_cols) * a.height + py0) * pic_w + (int64_t)(tile % a.atlas_cols) * a.width + x0;
    for (int i = tid; i < nr * nh; i += kWfThreads) {
        const int r = i / nh, k = i - r * nh;
        uint32_t px = 0u;
        if (tl.ofs >= 0) {
            const csdr_view_tap t = a.cols[x0 + k];
            px = tab[wf_scan_max(reinterpret_cast<const unsigned *>(span + r * a.chunks), t.first, t.first + t.count)];      // this pixel's bytes of the row in LDS
        }
        out[(int64_t)r * pic_w + k] = px;
    }
}

}  // namespace csdr
