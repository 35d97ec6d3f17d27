// kernels_waterfall.hpp -- the waterfall raster (gfx950): what WaterfallPanel does with every finished spectrum line.
//
//   quantise a line to one byte per point      src/panel/WaterfallPanel.cpp:64-72      wf_quantize
//   reverse the pending lines, write the runs  src/panel/WaterfallPanel.cpp:132-158    wf_update (the run table comes from the host)
//   index -> colour through the gradient       src/panel/WaterfallPanel.cpp:26-37,     wf_rgba
//     and the scrolled picture                 :186-213 (GL_REPEAT from waterfall_ofs)
//   the picture scaled to a W x H viewport     src/panel/WaterfallPanel.cpp:117-120,   wf_view_linear (GL_LINEAR / GL_REPEAT, the reference's picture)
//                                              :161-219                                wf_view_peak (the library's own: max over the footprint)
//
// Streaming kernels: every byte is read once and written once, so the target is the copy rate -- 16-byte accesses, no LDS beyond the 1 KB colour
// table (wave-uniform tables live in LDS in this project), no scratch.  The pending lines and both ring textures are kept with a row pitch that is
// a multiple of 16 bytes, so every row starts on a 16-byte boundary whatever fft_size / 2 is; a row's last fft_size / 2 % 16 bytes are written one
// by one.  The two viewport kernels read tap tables the host designs (design.hpp: view_columns / view_rows) -- no coordinate arithmetic on the device.
// A kernel is its own "which line, which row, which pixel" arithmetic around a body, and the bodies are __device__ __forceinline__ functions that
// kernels_wfbank.hpp (N panels per launch) calls too: wf_quantize_chunk, wf_stage_table, wf_store4, wf_linear4, wf_footprint_max, wf_scan_max
// (the row copy of wf_update / wfb_update and the pixel store of wf_rgba stay separate copies; wf_rgba's store and wf_store4 are one
// rule in two places: a change to the store-alignment rule goes to both).  None of the shared ones knows its caller; what differs between a
// panel and a bank arrives as data (an empty span, a null pointer, a base).
// Home unit: csdr_waterfall.hip.
#pragma once
#include "common.hpp"

#if defined(CSDR_TU_WATERFALL)
#define CSDR_KERNEL_WF CSDR_KERNEL
#else
#define CSDR_KERNEL_WF CSDR_KERNEL_ELSEWHERE
#endif

namespace csdr {

// DC-spike removal (SpectrumVisualProcessor.cpp:578-623): the points [start, end) within 2 kHz of the input centre are overwritten by their mirror
// images just outside that span -- point i in [start, half) takes point 2 start - 1 - i, point i in [half, end) takes point end + 1 + (i - half).
// The sources lie outside the span, so the in-place loops of the reference and a gather by index are the same thing.  start == end: nothing to do.
// csdr_spec_fetch applies it to its host copy, the waterfall's quantiser while it reads the points in HBM: ONE statement of the index arithmetic.
struct HideDcSpan { int start = 0, half = 0, end = 0; };
__host__ __device__ inline int hide_dc_source(const HideDcSpan &d, int i) {
    return (i < d.start || i >= d.end) ? i : (i < d.half ? 2 * d.start - 1 - i : d.end + 1 + (i - d.half));
}
// integer arithmetic as in the reference (host side)
inline HideDcSpan hide_dc_span(long long centerFreq, long long inFreq, long bandwidth, long long fftSize) {
    const HideDcSpan none;
    const long long freqMin = centerFreq - (bandwidth / 2), freqMax = centerFreq + (bandwidth / 2);
    const long long zeroPt = inFreq - freqMin;
    if (!(freqMin < inFreq && freqMax > inFreq)) return none;
    const int freqRange = (int)(freqMax - freqMin);
    const int freqStep = freqRange / (int)fftSize;
    if (freqStep == 0) return none;                                  // (the reference would divide by zero)
    int fftStart = (int)(zeroPt / freqStep) - (2000 / freqStep);
    int fftEnd = (int)(zeroPt / freqStep) + (2000 / freqStep);
    if (fftEnd - fftStart < 2) { fftEnd++; fftStart--; }
    const int numSteps = fftEnd - fftStart;
    if (!((fftEnd + numSteps / 2 + 1 < fftSize) && (fftStart - numSteps / 2 - 1 >= 0) && (fftEnd > fftStart))) return none;
    HideDcSpan d;
    d.start = fftStart; d.half = fftStart + (numSteps / 2); d.end = fftEnd;
    return d;
}

// WaterfallPanel.cpp:69-71: wv = v < 0 ? 0 : (v > 0.99 ? 0.99 : v) stored to a float, then (unsigned char)floor(wv * 255.0).  The comparison with 0.99
// is made in double and (float)0.99 = 0.99000000953... lies above 0.99 while its float predecessor lies below, so "v > 0.99" is "v >= 0.99f"; the
// clamp value is 0.99f and the largest index 252.  floor of the double product equals the truncated float product for every float in [0, 0.99f]
// (checked exhaustively by the tests against a float64 model); one multiply: nothing to contract.  -0 and every negative give 0; a NaN, for
// which the reference's conversion is undefined, gives 0 (the library's own definition, csdr_hip.h).
__device__ __forceinline__ unsigned wf_index(float v) {
    const float wv = v > 0.0f ? (v >= 0.99f ? 0.99f : v) : 0.0f;
    return (unsigned)(wv * 255.0f);
}

constexpr int kWfThreads = 256;
constexpr int kWfChunk = 16;                 // points (= bytes) per work-item of wf_quantize

struct WfQuantArgs {
    const float *src;                        // point p of line l: src[l * line_stride + (pair ? 2 p + 1 : p)]
    int64_t line_stride;                     // floats; 0: every line is the same one
    int pair;                                // 1: (x, y) pairs as in SpectrumVisualData, the y is used (:40-45); 0: plain values (:47)
    int wide;                                // 16-byte loads are possible: half % 16 == 0, the source and its line stride are 16-byte aligned
    int half, pitch;                         // bytes per row (fft_size / 2) and the rows' pitch
    uint8_t *pend[2];                        // the pending lines of both halves, rows of `pitch` bytes
    int row0, n_lines;                       // line l goes to pending row row0 + l
    int store;                               // 0: a dropped step (:60-62) -- only `keep` is written
    float *keep;                             // the panel's `points` (:39-49): receives the LAST line's values; nullptr: leave it
    HideDcSpan dc;                           // csdr_waterfall_step_spec with hideDC: the span to gather around
};

// One 16-point chunk of one line, the body of wf_quantize and wfb_quantize: points [p0, p0 + cnt) of `line` in either layout, gathered around `dc`
// (an empty span folds the gather away), packed to index bytes, stored to `row` (store false: a dropped step, :60-62) and as they are to
// keep[p0 ...] (`keep`: the panel's `points`; nullptr: not the line they receive).  wide_load / wide_keep: the chunk is whole and the line / `keep`
// can be accessed 16 bytes at a time.  `row` is 16-byte aligned: the pitch and the chunk's first byte are multiples of 16.  With store false
// `row` is not looked at and may be any address, one outside the pending rows included (the callers form it from the line's row number, which is
// -1 for a dropped step of the bank): it is only ever dereferenced under `store`.
__device__ __forceinline__ void wf_quantize_chunk(const float *line, bool pair, const HideDcSpan &dc, int p0, int cnt, bool wide_load, bool wide_keep,
                                                  bool store, uint8_t *row, float *keep) {
    float v[kWfChunk];
    if (wide_load) {
        if (pair) {
            const float4 *s = reinterpret_cast<const float4 *>(line + 2 * (int64_t)p0);
#pragma unroll
            for (int k = 0; k < 8; ++k) { float4 t = s[k]; pin_loaded(t); v[2 * k] = t.y; v[2 * k + 1] = t.w; }      // (pinned: whole 16-byte loads, not two 4-byte ones)
        } else {
            const float4 *s = reinterpret_cast<const float4 *>(line + p0);
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float4 t = s[k]; v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w; }
        }
    } else {
#pragma unroll
        for (int k = 0; k < kWfChunk; ++k) {
            const int p = hide_dc_source(dc, p0 + k);
            v[k] = k < cnt ? line[pair ? 2 * (int64_t)p + 1 : (int64_t)p] : 0.0f;
        }
    }
    if (store) {
        unsigned w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = wf_index(v[4 * q]) | (wf_index(v[4 * q + 1]) << 8) | (wf_index(v[4 * q + 2]) << 16) | (wf_index(v[4 * q + 3]) << 24);
        if (cnt == kWfChunk) *reinterpret_cast<int4 *>(row) = make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]);
        else {
#pragma unroll
            for (int k = 0; k < kWfChunk; ++k) if (k < cnt) row[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
    if (keep) {
        float *kp = keep + p0;
        if (wide_keep) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {        // (one vector value each: as four floats the last is merged with the last store below and the wide store split into 12 + 4 bytes)
                const csdr_f32x4 t = {v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
                reinterpret_cast<csdr_f32x4 *>(kp)[k] = t;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kWfChunk; ++k) if (k < cnt) kp[k] = v[k];
        }
    }
}

// grid (chunks of a half / 256, lines, 2 halves)
CSDR_KERNEL_WF __launch_bounds__(kWfThreads) void wf_quantize(WfQuantArgs a) {
    const int j = (int)blockIdx.z;
    const int i0 = ((int)blockIdx.x * kWfThreads + (int)threadIdx.x) * kWfChunk;
    if (i0 >= a.half) return;
    const int cnt = min(kWfChunk, a.half - i0);
    const int p0 = j * a.half + i0;                                   // byte i of half j comes from point j * half + i (:65-67)
    const bool in_dc = p0 < a.dc.end && p0 + kWfChunk > a.dc.start;   // the hideDC span is a handful of points: the items that meet it go point by point
    const bool wide = a.wide && cnt == kWfChunk;
    for (int l = (int)blockIdx.y; l < a.n_lines; l += (int)gridDim.y)
        wf_quantize_chunk(a.src + (int64_t)l * a.line_stride, a.pair != 0, a.dc, p0, cnt, wide && !in_dc, wide,
                          a.store != 0, a.pend[j] + (int64_t)(a.row0 + l) * a.pitch + i0, l == a.n_lines - 1 ? a.keep : nullptr);
}

// One run of WaterfallPanel::update (:139-158): ring rows [dst, dst + n) take the rows [src, src + n) of the REVERSED pending lines (:132-137), i.e.
// ring row dst + t takes pending row n_pending - 1 - src - t.
struct WfRun { int src, dst, n; };
struct WfUpdateArgs {
    WfRun run[2];                            // the runs whose rows survive the update, in the order the reference writes them (run[1] last)
    int n_runs, n_pending, pitch;
    uint8_t *ring[2];
    const uint8_t *pend[2];
};

// grid (16-byte chunks of a row / 256, rows of all runs, 2 halves): one launch per update whatever the number of runs
CSDR_KERNEL_WF __launch_bounds__(kWfThreads) void wf_update(WfUpdateArgs a) {
    const int j = (int)blockIdx.z;
    const int total = a.run[0].n + (a.n_runs > 1 ? a.run[1].n : 0);
    const int chunks = a.pitch / 16;
    for (int y = (int)blockIdx.y; y < total; y += (int)gridDim.y) {
        const int r = y < a.run[0].n ? 0 : 1, t = r ? y - a.run[0].n : y;
        const int dst = a.run[r].dst + t;
        // a row of the earlier run that the later run writes too: the reference's second glTexSubImage2D wins, so it is not written here at all
        if (r == 0 && a.n_runs > 1 && dst >= a.run[1].dst && dst < a.run[1].dst + a.run[1].n) continue;
        const int4 *s = reinterpret_cast<const int4 *>(a.pend[j] + (int64_t)(a.n_pending - 1 - a.run[r].src - t) * a.pitch);
        int4 *d = reinterpret_cast<int4 *>(a.ring[j] + (int64_t)dst * a.pitch);
        for (int c = (int)blockIdx.x * kWfThreads + (int)threadIdx.x; c < chunks; c += (int)gridDim.x * kWfThreads) d[c] = s[c];
    }
}

struct WfRgbaArgs {
    const uint8_t *ring[2];
    const uint32_t *table;                   // 256 x RGBA8 (byte order r, g, b, a), 16-byte aligned
    uint32_t *out;                           // [n_rows][2 * half] pixels, dense
    int half, pitch, lines, ofs, first_row, n_rows;
};

// The 256-entry colour table into the first 1 KB of the workgroup's LDS (every kernel that looks colours up); the caller's barrier follows.
__device__ __forceinline__ uint32_t *wf_stage_table(char *smem, const uint32_t *table) {
    uint32_t *tab = reinterpret_cast<uint32_t *>(smem);
    if (threadIdx.x < 64) reinterpret_cast<int4 *>(tab)[threadIdx.x] = reinterpret_cast<const int4 *>(table)[threadIdx.x];
    return tab;
}

// Pixels c[0 .. cnt) to out[base ...]: one 16-byte store if all four are there and the ADDRESS is on the 16-byte grid (`out` is 16-byte aligned, so
// `base` decides: a picture row whose length is no multiple of 4 leaves the next one off the grid), else one by one.  (A loop that stays a loop:
// unrolled, its last store is merged with the wide one, which is then split into a 12-byte and a 4-byte store.)
__device__ __forceinline__ void wf_store4(uint32_t *out, int64_t base, int cnt, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t *o = out + base;
    if (cnt == 4 && (base & 3) == 0) *reinterpret_cast<int4 *>(o) = make_int4((int)c0, (int)c1, (int)c2, (int)c3);
    else {
#pragma unroll 1
        for (int k = 0; k < cnt; ++k) o[k] = k == 0 ? c0 : (k == 1 ? c1 : (k == 2 ? c2 : c3));
    }
}

// grid (groups of 4 pixels of a half / 256, image rows, 2 halves).  Image row r is ring row (ofs + first_row + r) mod lines (:186-213: the texture
// coordinate runs from waterfall_ofs / lines under GL_REPEAT), half 0 then half 1.
CSDR_KERNEL_WF __launch_bounds__(kWfThreads) void wf_rgba(WfRgbaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t *tab = wf_stage_table(smem, a.table);
    __syncthreads();
    const int j = (int)blockIdx.z;
    const int q = (int)blockIdx.x * kWfThreads + (int)threadIdx.x;
    if (4 * q >= a.half) return;
    const int cnt = min(4, a.half - 4 * q);
    for (int r = (int)blockIdx.y; r < a.n_rows; r += (int)gridDim.y) {
        const int rr = (int)(((int64_t)a.ofs + a.first_row + r) % a.lines);
        const unsigned w = *reinterpret_cast<const unsigned *>(a.ring[j] + (int64_t)rr * a.pitch + 4 * q);     // inside the row's pitch even at its end
        const uint32_t c0 = tab[w & 0xffu], c1 = tab[(w >> 8) & 0xffu], c2 = tab[(w >> 16) & 0xffu], c3 = tab[w >> 24];
        const int64_t base = (int64_t)r * 2 * a.half + (int64_t)j * a.half + 4 * q;
        uint32_t *o = a.out + base;
        if (cnt == 4 && (base & 3) == 0) *reinterpret_cast<int4 *>(o) = make_int4((int)c0, (int)c1, (int)c2, (int)c3);
        else {
            // a row that does not start on a 16-byte boundary (half % 4 != 0), or its last pixels: one by one, as in wf_store4 -- whose text this is:
            // called from here, the loop came out two pixels at a time and the kernel 1.3 us slower per 512 x 65536 picture
#pragma unroll 1
            for (int k = 0; k < cnt; ++k) o[k] = k == 0 ? c0 : (k == 1 ? c1 : (k == 2 ? c2 : c3));
        }
    }
}

// ---- the viewport (csdr_hip.h, "Waterfall viewport"): a W x H picture of the ring from tap tables (csdr_view_tap, one per pixel column and row) ----
struct WfViewArgs {
    const uint8_t *ring[2];
    const uint32_t *table;                   // 256 x RGBA8, 16-byte aligned
    const csdr_view_tap *cols, *rows;        // [width], [height]
    uint32_t *out;                           // [height][width] pixels, dense
    int width, height, pitch, lines, ofs;
    // wf_view_peak: half 0 owns pixels [0, n0) in tiles0 tiles of tile0 pixels, half 1 the rest in tiles of tile1; `slots` 16-byte LDS slots per workgroup
    int n0, tiles0, tile0, tile1, slots;
};

// one channel-wise bilinear blend of table colours (csdr_hip.h): every operation rounded to float32 on its own, alpha 255
__device__ __forceinline__ uint32_t wf_blend(uint32_t c00, uint32_t c10, uint32_t c01, uint32_t c11, float al, float be) {
    uint32_t px = 0xff000000u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float a = (float)((c00 >> (8 * ch)) & 0xffu), b = (float)((c10 >> (8 * ch)) & 0xffu);
        const float c = (float)((c01 >> (8 * ch)) & 0xffu), d = (float)((c11 >> (8 * ch)) & 0xffu);
        // (rounded(): hipcc's __fmul_rn / __fadd_rn are plain operators, and a product next to a sum would be contracted into one fused operation)
        const float top = __fadd_rn(a, rounded(__fmul_rn(al, __fsub_rn(b, a))));
        const float bot = __fadd_rn(c, rounded(__fmul_rn(al, __fsub_rn(d, c))));
        const float m = __fadd_rn(top, rounded(__fmul_rn(be, __fsub_rn(bot, top))));
        px |= (uint32_t)__fadd_rn(m, 0.5f) << (8 * ch);              // m lies in [0, 255]: both blends stay between their end points
    }
    return px;
}

// LINEAR: four neighbouring pixels of one image row, the body of wf_view_linear and wfb_view_linear.  A gather: per pixel four byte reads (texels
// first, first + 1 of the column tap, in ring rows j0, j1 of the tap's half) and the blend.  ring0 / ring1: the two halves of one ring.
__device__ __forceinline__ void wf_linear4(const uint32_t *tab, const uint8_t *ring0, const uint8_t *ring1, int pitch, int lines, int ofs,
                                           const csdr_view_tap (&ct)[4], const csdr_view_tap rt, uint32_t (&c)[4]) {
    const int j0 = (int)(((int64_t)ofs + rt.first + lines) % lines), j1 = j0 + 1 == lines ? 0 : j0 + 1;                  // GL_REPEAT
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint8_t *tex = (ct[k].half ? ring1 : ring0) + ct[k].first;
        const uint8_t *r0 = tex + (int64_t)j0 * pitch, *r1 = tex + (int64_t)j1 * pitch;
        c[k] = wf_blend(tab[r0[0]], tab[r0[1]], tab[r1[0]], tab[r1[1]], ct[k].frac, rt.frac);
    }
}

// grid (groups of 4 pixels of a row / 256, image rows)
CSDR_KERNEL_WF __launch_bounds__(kWfThreads) void wf_view_linear(WfViewArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t *tab = wf_stage_table(smem, a.table);
    __syncthreads();
    const int px0 = 4 * ((int)blockIdx.x * kWfThreads + (int)threadIdx.x);
    if (px0 >= a.width) return;
    const int cnt = min(4, a.width - px0);
    csdr_view_tap ct[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) ct[k] = a.cols[min(px0 + k, a.width - 1)];
    for (int py = (int)blockIdx.y; py < a.height; py += (int)gridDim.y) {
        uint32_t c[4];
        wf_linear4(tab, a.ring[0], a.ring[1], a.pitch, a.lines, a.ofs, ct, a.rows[py], c);
        wf_store4(a.out, (int64_t)py * a.width + px0, cnt, c[0], c[1], c[2], c[3]);
    }
}

// byte-wise unsigned max of two words in plain integer arithmetic.  Bit 7 of each byte of d says whether the low 7 bits of x reach those of y (no
// borrow crosses a byte: 128 + xl - yl lies in [1, 255]); the top bits decide first.
__device__ __forceinline__ unsigned wf_max_u8x4(unsigned x, unsigned y) {
    const unsigned d = (x | 0x80808080u) - (y & 0x7f7f7f7fu);
    const unsigned ge = ((x & ~y) | (~(x ^ y) & d)) & 0x80808080u;
    const unsigned m = (ge >> 7) * 0xffu;                            // 0xff in every byte where x >= y
    return (x & m) | (y & ~m);
}
__device__ __forceinline__ int4 wf_max_u8x16(int4 x, int4 y) {
    return make_int4((int)wf_max_u8x4((unsigned)x.x, (unsigned)y.x), (int)wf_max_u8x4((unsigned)x.y, (unsigned)y.y),
                     (int)wf_max_u8x4((unsigned)x.z, (unsigned)y.z), (int)wf_max_u8x4((unsigned)x.w, (unsigned)y.w));
}
// the mask that keeps bytes [lo, hi) of a word (any lo, hi: clamped to 0 .. 4)
__device__ __forceinline__ unsigned wf_keep_bytes(int lo, int hi) {
    const unsigned below_hi = hi >= 4 ? 0xffffffffu : (hi <= 0 ? 0u : (1u << (8 * hi)) - 1u);
    const unsigned below_lo = lo >= 4 ? 0xffffffffu : (lo <= 0 ? 0u : (1u << (8 * lo)) - 1u);
    return below_hi & ~below_lo;
}
__device__ __forceinline__ int4 wf_keep_bytes16(int4 v, int lo, int hi) {
    return make_int4((int)((unsigned)v.x & wf_keep_bytes(lo, hi)), (int)((unsigned)v.y & wf_keep_bytes(lo - 4, hi - 4)),
                     (int)((unsigned)v.z & wf_keep_bytes(lo - 8, hi - 8)), (int)((unsigned)v.w & wf_keep_bytes(lo - 12, hi - 12)));
}

// PEAK, pass 1: the element-wise max of one 16-byte chunk (`col`: its place in ring row 0) over the `count` ring rows from row0 on, wrapping at
// `lines` (scrolled row r is ring row (ofs + r) mod lines)
__device__ __forceinline__ int4 wf_footprint_max(const uint8_t *col, int pitch, int lines, int row0, int count) {
    int rr = row0;
    int4 m = *reinterpret_cast<const int4 *>(col + (int64_t)rr * pitch);
    for (int r = 1; r < count; ++r) {
        if (++rr == lines) rr = 0;
        m = wf_max_u8x16(m, *reinterpret_cast<const int4 *>(col + (int64_t)rr * pitch));
    }
    return m;
}
// PEAK, pass 2: the largest of the LDS bytes [s, e) of `words`, word by word
__device__ __forceinline__ unsigned wf_scan_max(const unsigned *words, int s, int e) {
    unsigned best = 0;
    for (int w = s >> 2; 4 * w < e; ++w) {
        const unsigned x = words[w] & wf_keep_bytes(s - 4 * w, e - 4 * w);
        best = max(best, max(max(x & 0xffu, (x >> 8) & 0xffu), max((x >> 16) & 0xffu, x >> 24)));
    }
    return best;
}

// grid (tiles of both halves, image rows).  A workgroup owns up to 256 consecutive pixels of one half in one image row; tiles end on footprint
// boundaries, so no footprint straddles two of them.  Pass 1: the element-wise max of the footprint's ring rows over the tile's texel span, in
// 16-byte loads (rows have a 16-byte pitch), into LDS; the bytes outside the span are cleared.  One barrier.  Pass 2: each work-item scans its pixel's
// bytes in LDS word by word and looks the colour of the largest up.  The max is separable, so every texel is read once.  A single pixel whose
// span does not fit the slots (the host then makes the tile that one pixel) is folded: slot s holds the max of chunks s, s + slots, ...
CSDR_KERNEL_WF __launch_bounds__(kWfThreads) void wf_view_peak(WfViewArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t *tab = wf_stage_table(smem, a.table);
    int4 *span = reinterpret_cast<int4 *>(smem + 256 * sizeof(uint32_t));
    const int tid = (int)threadIdx.x;
    const int h = (int)blockIdx.x >= a.tiles0 ? 1 : 0;
    const int per = h ? a.tile1 : a.tile0, nh = h ? a.width - a.n0 : a.n0;
    const int k0 = (h ? (int)blockIdx.x - a.tiles0 : (int)blockIdx.x) * per;
    const int kn = min(per, nh - k0);                                 // pixels of this tile (>= 1)
    const csdr_view_tap *cols = a.cols + (h ? a.n0 : 0) + k0;
    const csdr_view_tap rt = a.rows[blockIdx.y];
    const int t0 = cols[0].first, t1 = cols[kn - 1].first + cols[kn - 1].count;         // the tile's texel span [t0, t1)
    const int c0 = t0 >> 4, nchunks = ((t1 + 15) >> 4) - c0;
    const bool fold = nchunks > a.slots;
    const int nslots = fold ? a.slots : nchunks;
    const uint8_t *ring = (h ? a.ring[1] : a.ring[0]) + 16 * (int64_t)c0;
    const int row0 = (int)(((int64_t)a.ofs + rt.first) % a.lines);    // scrolled row r is ring row (ofs + r) mod lines
    for (int s = tid; s < nslots; s += kWfThreads) {
        int4 acc = make_int4(0, 0, 0, 0);
        for (int cc = s; cc < nchunks; cc += a.slots) {               // (a second turn only when folded)
            int4 m = wf_footprint_max(ring + 16 * (int64_t)cc, a.pitch, a.lines, row0, rt.count);
            if (cc == 0) m = wf_keep_bytes16(m, t0 - 16 * c0, 16);
            if (cc == nchunks - 1) m = wf_keep_bytes16(m, 0, t1 - 16 * (c0 + cc));
            acc = wf_max_u8x16(acc, m);
        }
        span[s] = acc;
    }
    __syncthreads();
    if (tid >= kn) return;
    const csdr_view_tap t = cols[tid];
    const int s = fold ? 0 : t.first - 16 * c0, e = fold ? 16 * nslots : s + t.count;   // this pixel's bytes in LDS
    a.out[(int64_t)blockIdx.y * a.width + (h ? a.n0 : 0) + k0 + tid] = tab[wf_scan_max(reinterpret_cast<const unsigned *>(span), s, e)];
}

}  // namespace csdr
