// kernels_distrib.hpp -- the waterfall feed (gfx950): what FFTDataDistributor does with the samples of one popped input.
//
//   append the block behind what is buffered        src/process/FFTDataDistributor.cpp:66-84     (no copy: the block is read where it lies)
//   copy every emitted line out of the buffer       src/process/FFTDataDistributor.cpp:112-121   distrib_gather, segments 0 .. n_lines - 1
//   move the unconsumed samples to the front        src/process/FFTDataDistributor.cpp:133-141   distrib_gather, segment n_lines
//
// The reference keeps 0.25 s of samples and moves them with memcpy / memmove; after every input fewer than fftSize samples stay buffered, so here
// the buffer is the virtual stream V = carry[0 : buffered) ++ block[0 : n_add): the carried partial line and the caller's block in place.  Which
// lines go out is decided on the host (integer and double arithmetic, csdr_distrib.hip); the kernel only moves samples.
//
// A streaming copy: every byte is read once and written once, so the target is the copy rate -- 16-byte accesses, no LDS, no scratch.  A sample
// is 8 bytes, so a segment can start 8 bytes off a 16-byte boundary on either side.  A work-item owns 16-byte ALIGNED pieces of the destination
// (the first and the last piece of a segment may hold one sample only); its two samples are read with one 16-byte load where the source address
// is 16-byte aligned too and both lie on the same side of the carry / block boundary, else with two 8-byte loads, each from its own side.
// Home unit: csdr_distrib.hip.
#pragma once
#include "common.hpp"

#if defined(CSDR_TU_DISTRIB)
#define CSDR_KERNEL_DG CSDR_KERNEL
#else
#define CSDR_KERNEL_DG CSDR_KERNEL_ELSEWHERE
#endif

namespace csdr {

constexpr int kDgThreads = 256;
constexpr int kDgPieces = 4;                 // 16-byte pieces per work-item: all loads are issued before the first store

struct DistribArgs {
    const float2 *carry_in;                  // V[0 : buffered); 16-byte aligned
    const float2 *block;                     // V[buffered : buffered + n_add); 8-byte aligned
    float2 *lines;                           // [n_lines][fft], dense; 16-byte aligned
    float2 *carry_out;                       // receives V[tail_start : tail_start + tail_len); 16-byte aligned, never carry_in
    const int *starts;                       // [n_lines]: index in V of the first sample of every emitted line
    int buffered, fft, n_lines;
    int tail_start, tail_len;
};

// One 16-byte load that stays one: written as a plain float4 load, the compiler shares its lower half with the 8-byte path's first load and
// fetches the upper half word by word.  The streaming hint fits as well: every source byte is read once.
__device__ __forceinline__ float4 dg_load16(const float2 *p) {
#if defined(__AMDGCN__)
    typedef float dg_f4 __attribute__((ext_vector_type(4)));
    const dg_f4 t = __builtin_nontemporal_load(reinterpret_cast<const dg_f4 *>(p));
    return make_float4(t.x, t.y, t.z, t.w);
#else
    return *reinterpret_cast<const float4 *>(p);
#endif
}
__device__ __forceinline__ float2 dg_sample(const DistribArgs &a, int v) { return v < a.buffered ? a.carry_in[v] : a.block[v - a.buffered]; }

// grid (pieces of the longest segment / (256 * kDgPieces), segments): segment l < n_lines is line l, segment n_lines the new carry
CSDR_KERNEL_DG __launch_bounds__(kDgThreads) void distrib_gather(DistribArgs a) {
    for (int seg = (int)blockIdx.y; seg <= a.n_lines; seg += (int)gridDim.y) {
        const bool tail = seg == a.n_lines;
        const int s = tail ? a.tail_start : a.starts[seg];
        const int len = tail ? a.tail_len : a.fft;
        float2 *dst = tail ? a.carry_out : a.lines + (int64_t)seg * a.fft;
        const int pd = (int)(((uintptr_t)dst >> 3) & 1);              // 1: the segment starts in the upper half of a 16-byte piece
        const int pieces = (len + pd + 1) >> 1;                       // piece q holds the segment's samples 2 q - pd and 2 q - pd + 1
        const int q0 = (int)blockIdx.x * (kDgThreads * kDgPieces) + (int)threadIdx.x;
        float4 v[kDgPieces];
#pragma unroll
        for (int u = 0; u < kDgPieces; ++u) {
            const int q = q0 + u * kDgThreads, j = 2 * q - pd;
            v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (q >= pieces) continue;
            const bool lo = j >= 0, hi = j + 1 < len;
            const int i = s + j;                                       // V index of the piece's lower sample
            if (lo && hi) {
                const float2 *p = i < a.buffered ? a.carry_in + i : a.block + (i - a.buffered);
                if (i + 1 != a.buffered && ((uintptr_t)p & 15) == 0) v[u] = dg_load16(p);
                else { const float2 x = *p, y = dg_sample(a, i + 1); v[u] = make_float4(x.x, x.y, y.x, y.y); }
            } else if (lo) { const float2 x = dg_sample(a, i); v[u].x = x.x; v[u].y = x.y; }
            else if (hi) { const float2 y = dg_sample(a, i + 1); v[u].z = y.x; v[u].w = y.y; }
        }
#pragma unroll
        for (int u = 0; u < kDgPieces; ++u) {
            const int q = q0 + u * kDgThreads, j = 2 * q - pd;
            if (q >= pieces) continue;
            const bool lo = j >= 0, hi = j + 1 < len;
            if (lo && hi) *reinterpret_cast<float4 *>(dst + j) = v[u];
            else if (lo) dst[j] = make_float2(v[u].x, v[u].y);
            else if (hi) dst[j + 1] = make_float2(v[u].z, v[u].w);
        }
    }
}

}  // namespace csdr
