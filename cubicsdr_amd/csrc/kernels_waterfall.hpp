// kernels_waterfall.hpp -- the waterfall raster (gfx950): what WaterfallPanel does with every finished spectrum line.
//
//   quantise a line to one byte per point      src/panel/WaterfallPanel.cpp:64-72      wf_quantize
//   reverse the pending lines, write the runs  src/panel/WaterfallPanel.cpp:132-158    wf_update (the run table comes from the host)
//   index -> colour through the gradient       src/panel/WaterfallPanel.cpp:26-37,     wf_rgba
//     and the scrolled picture                 :186-213 (GL_REPEAT from waterfall_ofs)
//
// Streaming kernels: every byte is read once and written once, so the target is the copy rate -- 16-byte accesses, no LDS beyond the 1 KB colour
// table (wave-uniform tables live in LDS in this project), no scratch.  The pending lines and both ring textures are kept with a row pitch that is
// a multiple of 16 bytes, so every row starts on a 16-byte boundary whatever fft_size / 2 is; a row's last fft_size / 2 % 16 bytes are written one
// by one.  Home unit: csdr_waterfall.hip.
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

// grid (chunks of a half / 256, lines, 2 halves)
CSDR_KERNEL_WF __launch_bounds__(kWfThreads) void wf_quantize(WfQuantArgs a) {
    const int j = (int)blockIdx.z;
    const int i0 = ((int)blockIdx.x * kWfThreads + (int)threadIdx.x) * kWfChunk;
    if (i0 >= a.half) return;
    const int cnt = min(kWfChunk, a.half - i0);
    const int p0 = j * a.half + i0;                                   // byte i of half j comes from point j * half + i (:65-67)
    const bool in_dc = p0 < a.dc.end && p0 + kWfChunk > a.dc.start;   // the hideDC span is a handful of points: the items that meet it go point by point
    for (int l = (int)blockIdx.y; l < a.n_lines; l += (int)gridDim.y) {
        const float *line = a.src + (int64_t)l * a.line_stride;
        float v[kWfChunk];
        if (a.wide && cnt == kWfChunk && !in_dc) {
            if (a.pair) {
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
                const int p = hide_dc_source(a.dc, p0 + k);
                v[k] = k < cnt ? line[a.pair ? 2 * (int64_t)p + 1 : (int64_t)p] : 0.0f;
            }
        }
        if (a.store) {
            unsigned w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = wf_index(v[4 * q]) | (wf_index(v[4 * q + 1]) << 8) | (wf_index(v[4 * q + 2]) << 16) | (wf_index(v[4 * q + 3]) << 24);
            uint8_t *row = a.pend[j] + (int64_t)(a.row0 + l) * a.pitch + i0;          // 16-byte aligned: pitch % 16 == 0, i0 % 16 == 0
            if (cnt == kWfChunk) *reinterpret_cast<int4 *>(row) = make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]);
            else {
#pragma unroll
                for (int k = 0; k < kWfChunk; ++k) if (k < cnt) row[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            }
        }
        if (a.keep && l == a.n_lines - 1) {
            float *kp = a.keep + p0;
            if (a.wide && cnt == kWfChunk) {
#pragma unroll
                for (int k = 0; k < 4; ++k) reinterpret_cast<float4 *>(kp)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < kWfChunk; ++k) if (k < cnt) kp[k] = v[k];
            }
        }
    }
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

// grid (groups of 4 pixels of a half / 256, image rows, 2 halves).  Image row r is ring row (ofs + first_row + r) mod lines (:186-213: the texture
// coordinate runs from waterfall_ofs / lines under GL_REPEAT), half 0 then half 1.
CSDR_KERNEL_WF __launch_bounds__(kWfThreads) void wf_rgba(WfRgbaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(smem);
    if (threadIdx.x < 64) reinterpret_cast<int4 *>(tab)[threadIdx.x] = reinterpret_cast<const int4 *>(a.table)[threadIdx.x];
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
            // a row that does not start on a 16-byte boundary (half % 4 != 0), or its last pixels: one by one.  (A loop that stays a loop: unrolled,
            // its last store is merged with the wide one above, which is then split into a 12-byte and a 4-byte store.)
#pragma unroll 1
            for (int k = 0; k < cnt; ++k) o[k] = k == 0 ? c0 : (k == 1 ? c1 : (k == 2 ? c2 : c3));
        }
    }
}

}  // namespace csdr
