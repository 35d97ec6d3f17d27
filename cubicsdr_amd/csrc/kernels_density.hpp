// kernels_density.hpp -- the density bank (gfx950): how often the trace passed through every pixel of a tile, one uint32 grid per slot in HBM.
//
//   the cover of a chunk of frames               density_cover   (one work-item per column; a difference array in LDS, a prefix sum down the rows)
//   decay, weight, saturating add, block maxima  density_fold    (sums the chunk planes in fixed order)
//   counts -> palette -> RGBA8 atlas             density_render  (reduces the slot's block maxima; 16 bytes per work-item)
//
// The picture is the library's own definition (include/csdr_hip.h, "Density bank"); its arithmetic is stated once in density_host.hpp, on top of
// trace_host.hpp, and called from here.  A step is ONE launch of density_cover and ONE of density_fold for all items, a render ONE launch for all
// views: a record per item (DnJob) or per tile (csdr_density_view), uploaded with the call, says what to do.  No atomics: a column of the
// difference array belongs to one work-item, a cell of a slot to one work-item of density_fold, and maxima are reduced by lane exchange.
// Home unit: csdr_density.hip.
#pragma once
#include "common.hpp"
#include "kernels_waterfall.hpp"
#include "density_host.hpp"

#if defined(CSDR_TU_DENSITY)
#define CSDR_KERNEL_DENSITY CSDR_KERNEL
#else
#define CSDR_KERNEL_DENSITY CSDR_KERNEL_ELSEWHERE
#endif

namespace csdr {

constexpr int kDnCols = 64;                  // columns of a tile to a workgroup of every kernel here: one wave of density_cover, 256 bytes of a row
constexpr int kDnChunk = 32;                 // frames to a workgroup of density_cover: 953 frames of a 1920-wide slot are 30 x 30 workgroups, and a
                                             // workgroup's fixed cost (clearing and summing height rows) is spread over 32 frames' vertices
constexpr int kDnBand = 448;                 // rows of a tile to a workgroup of density_cover (even): 57 KiB of LDS at most, below the 64 KiB a
                                             // launch gets without asking; a taller tile's workgroups each repeat the intervals for their band
constexpr int kDnThreads = 256;              // density_fold, density_render
constexpr int kDnFoldRows = 2 * (kDnThreads / (kDnCols / 4));       // rows to a workgroup of density_fold: a work-item owns 4 columns of 2 rows
constexpr int kDnRenderRows = 64;            // rows to a workgroup of density_render

// One item of a step.  Chunk k of the item covers frames [k kDnChunk, (k + 1) kDnChunk) and owns plane k: Hp x Wp words behind `plane0`, the
// word at [j][c] holding the cover of rows 2 j (low half) and 2 j + 1 (high half) of column c -- a chunk's cover is at most kDnChunk.
struct DnJob {
    const float *pts;          // device memory: the caller's, or the staged copy of host points; nullptr with n_chunks == 0
    int64_t frame_stride;      // floats from a frame to the next
    int64_t plane0;            // words
    int32_t slot, n, stride;   // vertices per frame; floats from one vertex to the next (1 + layout)
    int32_t frames, kind, n_chunks;
    HideDcSpan dc;             // vertex i reads point hide_dc_source(dc, i)
    uint32_t keep_q16, weight;
};
static_assert(sizeof(DnJob) == 72, "DnJob layout");

struct DnArgs {
    const DnJob *jobs;
    uint32_t *planes;
    uint32_t *count;           // [max_slots][H][W]
    uint32_t *blockmax;        // [max_slots][col_blocks * fold_groups]
    int W, H, Wp, Hp;          // Wp = col_blocks * kDnCols, Hp = ceil(H / 2)
    int col_blocks, bands, fold_groups;
};

// words of a column's difference array: the rows of the tallest band + 1 entries, two to a word; and the LDS of a workgroup with the windows behind
__host__ __device__ inline int dn_cover_words(int H) { return (H < kDnBand ? H : kDnBand) / 2 + 1; }
inline size_t dn_cover_lds(int H) { return ((size_t)dn_cover_words(H) + 2) * kDnCols * sizeof(uint32_t); }

// delta added, modulo 2^16, to one half of a word; the other half stays (the word is read and written as a word: one type for the array)
__device__ __forceinline__ void dn_add16(uint32_t *word, int half, uint32_t delta) {
    const uint32_t w = *word, sh = 16u * (uint32_t)half, mask = 0xffffu << sh;
    *word = (w & ~mask) | ((w + (delta << sh)) & mask);
}

// grid (items * col_blocks * bands, chunks of the longest item), kDnCols work-items.  A work-item owns column c of the tile and the column's
// entries of a difference array of the band's rows + 1 in LDS: 16-bit entries, rows 2 j and 2 j + 1 in the two halves of word [j][lane], so that the
// lanes of the wave fall into 64 different banks whatever rows they touch.  For every frame of the chunk it forms [lo, hi] (density_interval),
// cut to the band, and adds 1 at lo and -1 behind hi, modulo 2^16; the running sum down the rows is the chunk's cover, at most kDnChunk, and goes to
// the chunk's plane two rows to a word.  Nothing is shared between work-items: no barrier.
CSDR_KERNEL_DENSITY __launch_bounds__(kDnCols) void density_cover(DnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int per_job = a.col_blocks * a.bands;
    const DnJob jb = a.jobs[blockIdx.x / (unsigned)per_job];
    const int chunk = (int)blockIdx.y;
    if (chunk >= jb.n_chunks) return;
    const int rem = (int)(blockIdx.x % (unsigned)per_job), cb = rem / a.bands, band = rem % a.bands;
    const int lane = (int)threadIdx.x, c = cb * kDnCols + lane;
    const int b0 = band * kDnBand, rows = min(kDnBand, a.H - b0), nw = rows / 2 + 1;      // rows + 1 entries
    uint32_t *words = reinterpret_cast<uint32_t *>(smem);                                 // [dn_cover_words(H)][kDnCols]
    float *win = reinterpret_cast<float *>(words + dn_cover_words(a.H) * kDnCols) + 2 * lane;
    for (int j = 0; j < nw; ++j) words[j * kDnCols + lane] = 0u;
    uint32_t *mine = words + lane;                                                        // entry of row r: half r & 1 of mine[(r >> 1) kDnCols]
    if (c < a.W) {
        const int64_t v0 = trace_first_vertex(c, jb.n, a.W), v1 = trace_first_vertex((int64_t)c + 1, jb.n, a.W);
        const int f1 = min(jb.frames, (chunk + 1) * kDnChunk);
        for (int f = chunk * kDnChunk; f < f1; ++f) {
            const TracePoly pl = trace_poly(jb.pts + (int64_t)f * jb.frame_stride, nullptr, jb.n, jb.stride, jb.kind, a.H, 0);
            int lo, hi;
            density_interval(pl, jb.dc, a.W, c, v0, v1, win, lo, hi);
            if (hi < b0 || lo >= b0 + rows) continue;
            const int s = max(lo, b0) - b0, e = min(hi + 1, b0 + rows) - b0;
            dn_add16(mine + (s >> 1) * kDnCols, s & 1, 1u);
            dn_add16(mine + (e >> 1) * kDnCols, e & 1, 0xffffu);
        }
    }
    uint32_t *plane = a.planes + jb.plane0 + ((int64_t)chunk * a.Hp + b0 / 2) * a.Wp + c;
    uint32_t acc = 0;
    for (int j = 0; j < (rows + 1) / 2; ++j) {
        const uint32_t w = words[j * kDnCols + lane];
        acc = (acc + (w & 0xffffu)) & 0xffffu;
        const uint32_t low = acc;
        acc = (acc + (w >> 16)) & 0xffffu;
        plane[(int64_t)j * a.Wp] = low | (acc << 16);        // (an odd band's last high half is row `rows`: nobody reads it)
    }
}

// 4 cells of a dense row: one 16-byte access where the address is on the 16-byte grid, as wf_store4
__device__ __forceinline__ int4 dn_load4(const uint32_t *p, int64_t base, int cnt) {
    const uint32_t *q = p + base;
    if (cnt == 4 && (base & 3) == 0) return *reinterpret_cast<const int4 *>(q);
    int4 v = make_int4(0, 0, 0, 0);
    if (cnt > 0) v.x = (int)q[0];
    if (cnt > 1) v.y = (int)q[1];
    if (cnt > 2) v.z = (int)q[2];
    if (cnt > 3) v.w = (int)q[3];
    return v;
}

// grid (items * col_blocks, fold_groups).  A work-item owns columns [c, c + 4) of rows 2 j and 2 j + 1: it sums its words of the item's planes in
// chunk order (16-byte loads; the planes are padded to whole column blocks), steps its 8 cells (density_step_cell) and stores them.  The
// workgroup's maximum goes to blockmax[slot][cb * fold_groups + group]: lane exchange, then one value per wave through LDS.
CSDR_KERNEL_DENSITY __launch_bounds__(kDnThreads) void density_fold(DnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *wave_max = reinterpret_cast<uint32_t *>(smem);          // [kDnThreads / 64]
    const DnJob jb = a.jobs[blockIdx.x / (unsigned)a.col_blocks];
    const int cb = (int)(blockIdx.x % (unsigned)a.col_blocks), tid = (int)threadIdx.x;
    const int c = cb * kDnCols + 4 * (tid & (kDnCols / 4 - 1)), cnt = min(4, a.W - c);
    const int j = (int)blockIdx.y * (kDnFoldRows / 2) + tid / (kDnCols / 4);
    uint32_t mx = 0;
    if (cnt > 0 && 2 * j < a.H) {
        uint32_t cov[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        const uint32_t *pw = a.planes + jb.plane0 + (int64_t)j * a.Wp + c;
        for (int k = 0; k < jb.n_chunks; ++k) {
            const int4 w = *reinterpret_cast<const int4 *>(pw + (int64_t)k * a.Hp * a.Wp);
            const uint32_t u[4] = {(uint32_t)w.x, (uint32_t)w.y, (uint32_t)w.z, (uint32_t)w.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) { cov[0][q] += u[q] & 0xffffu; cov[1][q] += u[q] >> 16; }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = 2 * j + h;
            if (r >= a.H) break;
            const int64_t base = ((int64_t)jb.slot * a.H + r) * a.W + c;
            const int4 old = dn_load4(a.count, base, cnt);
            const uint32_t o[4] = {(uint32_t)old.x, (uint32_t)old.y, (uint32_t)old.z, (uint32_t)old.w};
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] = density_step_cell(o[q], jb.keep_q16, jb.weight, cov[h][q]);
                if (q < cnt) mx = max(mx, v[q]);
            }
            wf_store4(a.count, base, cnt, v[0], v[1], v[2], v[3]);
        }
    }
    for (int o = 1; o < 64; o <<= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    if ((tid & 63) == 0) wave_max[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kDnThreads / 64; ++w) mx = max(mx, wave_max[w]);
        a.blockmax[(int64_t)jb.slot * (a.col_blocks * a.fold_groups) + cb * a.fold_groups + (int)blockIdx.y] = mx;
    }
}

struct DnRenderArgs {
    const csdr_density_view *views;        // [tile rows * atlas_cols]: the unused tiles of the last tile row have slot -1
    const uint32_t *count, *blockmax, *palette;
    uint32_t *out;             // [tile rows * H][atlas_cols * W] pixels, dense
    int W, H, atlas_cols, col_blocks, n_blocks;      // n_blocks: block maxima per slot
};

// grid (tiles * col_blocks, groups of kDnRenderRows rows).  The palette goes to LDS (wave-uniform tables live in LDS in this project), the
// slot's block maxima are reduced to its peak -- every workgroup of the tile repeats that: a few hundred values against 16 KiB of pixels -- and every
// work-item maps 4 counts of a row at a time (density_index) and stores 16 bytes.
CSDR_KERNEL_DENSITY __launch_bounds__(kDnThreads) void density_render(DnRenderArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t *tab = wf_stage_table(smem, a.palette);
    uint32_t *wave_max = reinterpret_cast<uint32_t *>(smem + 256 * sizeof(uint32_t));     // [kDnThreads / 64]
    const int tile = (int)(blockIdx.x / (unsigned)a.col_blocks), cb = (int)(blockIdx.x % (unsigned)a.col_blocks), tid = (int)threadIdx.x;
    const csdr_density_view vw = a.views[tile];
    uint32_t full = vw.full;
    if (vw.slot >= 0 && full == 0) {                      // (uniform over the workgroup)
        uint32_t mx = 0;
        for (int i = tid; i < a.n_blocks; i += kDnThreads) mx = max(mx, a.blockmax[(int64_t)vw.slot * a.n_blocks + i]);
        for (int o = 1; o < 64; o <<= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
        if ((tid & 63) == 0) wave_max[tid >> 6] = mx;
        __syncthreads();
        full = 1;
        for (int w = 0; w < kDnThreads / 64; ++w) full = max(full, wave_max[w]);
    } else __syncthreads();                               // the palette
    const int px0 = cb * kDnCols + 4 * (tid & (kDnCols / 4 - 1)), cnt = min(4, a.W - px0);
    if (cnt <= 0) return;
    const int r1 = min(a.H, ((int)blockIdx.y + 1) * kDnRenderRows);
    const int64_t pic_w = (int64_t)a.atlas_cols * a.W;
    for (int r = (int)blockIdx.y * kDnRenderRows + tid / (kDnCols / 4); r < r1; r += kDnThreads / (kDnCols / 4)) {
        uint32_t px[4] = {0u, 0u, 0u, 0u};
        if (vw.slot >= 0) {
            const int4 v = dn_load4(a.count, ((int64_t)vw.slot * a.H + r) * a.W + px0, cnt);
            px[0] = tab[density_index((uint32_t)v.x, full)]; px[1] = tab[density_index((uint32_t)v.y, full)];
            px[2] = tab[density_index((uint32_t)v.z, full)]; px[3] = tab[density_index((uint32_t)v.w, full)];
        }
        wf_store4(a.out, ((int64_t)(tile / a.atlas_cols) * a.H + r) * pic_w + (int64_t)(tile % a.atlas_cols) * a.W + px0, cnt, px[0], px[1], px[2], px[3]);
    }
}

}  // namespace csdr
