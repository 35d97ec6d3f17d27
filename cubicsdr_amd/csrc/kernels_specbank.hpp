// kernels_specbank.hpp -- N independent SpectrumVisualProcessors in one launch (csdr_specbank, include/csdr_hip.h "Spectrum bank").
//
// Replaces, per slot and per process() input (reference file:line, src/process/SpectrumVisualProcessor.cpp):
//   the reset of fft_result_peak / fft_ceil_peak / fft_floor_peak  :264-273   (which input it falls in front of: the host's countdown)
//   frame selection                                                 :387-421   (which branch: the host, from the lengths alone; the copies: here)
//   fft_execute                                                     :439       (lds_fft of kernels_spec.hpp, 2 * fftSize <= 4096 points in LDS)
//   float magnitude with the half swap                              :441-452
//   NaN re-seeding, the two double averagers, ceiling / floor       :494-505
//   running peak                                                    :506-510, :523-530
//   the four trackers at 0.05                                       :513-521
//   display points, two bins per point (visualRatio 1)              :532-576, :626-627
// One workgroup per slot walks that slot's job records in order: the averagers and trackers are recurrences over a slot's frames, and slots
// share nothing.  The kernel is latency-bound: a frame moves about 100 KB of a slot's state, and the chain of radix passes with their barriers
// is what takes the time; the parallelism is across slots.
// All LDS is dynamic (`smem`): 2 * Fi float2 (ping-pong of the transform) + 8 doubles of reduction scratch.
// The per-frame statements are __device__ functions (sb_peak_reset .. sb_store_meta) that viewbank_process calls too; what the two kernels do not
// share is their point loop: two fixed bins per point here, the view map and the hideDC gather there.
#pragma once
#include "common.hpp"
#include "stream_order.hpp"
#include "kernels_spec.hpp"

#if defined(CSDR_TU_SPECBANK)
#define CSDR_KERNEL_SB CSDR_KERNEL
#else
#define CSDR_KERNEL_SB CSDR_KERNEL_ELSEWHERE
#endif

namespace csdr {

constexpr int kSbPrime = 0, kSbSlide = 1, kSbFull = 2;

struct SpecBankJob {             // one non-empty process() input of a slot
    const float2 *src;           // the input's samples (device memory)
    int32_t n;                   // samples read from src: min(input length, Fi)
    int32_t action;              // kSbPrime | kSbSlide | kSbFull
    int32_t arg;                 // PRIME: num_copy (:408-411).  SLIDE: lastDataSize - (Fi - n), the first kept sample of fftLastData (:416)
    int32_t frame;               // output frame of the slot in this call; -1: none (PRIME)
    int32_t do_peak;             // doPeak of this input (:247)
    int32_t peak_reset_now;      // peakReset reached 0 in front of this input (:264-273)
};
static_assert(sizeof(SpecBankJob) == 32, "SpecBankJob layout");
using SpecBankRun = SlotRun;                                             // one workgroup: jobs [job0, job0 + n_jobs) of `slot`
struct SpecBankTrk { double ceil_ma, ceil_maa, floor_ma, floor_maa, ceil_peak, floor_peak; };
struct SpecBankFrame { double point_ceil, point_floor; int32_t hold, pad; };   // hold: the frame carries spectrum_hold_points

struct SpecBankArgs {
    const SpecBankRun *runs;
    const SpecBankJob *jobs;
    const float2 *tw4096;
    float2 *last;                // [slots][Fi]  fftLastData
    double *ma, *maa, *peak;     // [slots][Fi]  fft_result_ma / _maa / _peak, in the order of fft_result (after the half swap)
    SpecBankTrk *trk;            // [slots]
    float *points, *hold;        // [slots][max_frames][F]  y of every display point / hold point
    SpecBankFrame *meta;         // [slots][max_frames]
    int32_t Fi, max_frames;
    double rate;                 // fft_average_rate (a float member: the host widens it)
    float sf;                    // scaleFactor
};

__host__ __device__ constexpr size_t specbank_lds_bytes(int Fi) { return (size_t)2 * Fi * sizeof(float2) + 8 * sizeof(double); }

// ---- the per-frame statements of one SpectrumVisualProcessor, stated once for specbank_process and viewbank_process (kernels_viewbank.hpp).  Every
// function is called by whole workgroups of kFftThreads (the barriers inside are reached by all threads); a work-item's index is threadIdx.x.

// :266-272, with the trackers as they stand in front of this input
__device__ __forceinline__ void sb_peak_reset(double *peak, SpecBankTrk &t, int Fi) {
    for (int i = threadIdx.x; i < Fi; i += kFftThreads) peak[i] = t.floor_maa;
    t.ceil_peak = t.floor_maa;
    t.floor_peak = t.ceil_maa;
}

// priming (:407-413): the first n samples of `fresh` followed by zeros, num_copy in all
__device__ __forceinline__ void sb_prime(float2 *last, const float2 *fresh, int n, int num_copy) {
    for (int i = threadIdx.x; i < num_copy; i += kFftThreads) last[i] = i < n ? fresh[i] : make_float2(0.f, 0.f);
    __syncthreads();                                                       // the next job reads `last` (and `peak`) across threads
}

// fftInput (:401-404, :415-418) into LDS -- what is kept of fftLastData from `first_kept` on, then the n samples of `fresh` (n == Fi: FULL) -- and its
// transform; it becomes fftLastData once every thread has read what it keeps of the old one
__device__ __forceinline__ const float2 *sb_transform(float2 *last, const float2 *fresh, int n, int first_kept, int Fi, float2 *sa, float2 *sb,
                                                      const float2 *tw4096) {
    const int tid = threadIdx.x;
    const int keep = Fi - n;                                               // 0 for FULL
    for (int i = tid; i < Fi; i += kFftThreads) sa[i] = i < keep ? last[first_kept + i] : fresh[i - keep];
    __syncthreads();
    for (int i = tid; i < Fi; i += kFftThreads) last[i] = sa[i];
    return lds_fft(sa, sb, Fi, tw4096);
}

// fft_result[i] = |X[(i + Fi / 2) mod Fi]| in float (:441-452); the averagers (:494-498); ceiling, floor, peak (:500-510); the trackers (:513-521) and
// the held extremes (:523-530).  A thread takes two adjacent bins: those of a full-span display point (:542-561).  s_red: [2][4 waves]
__device__ __forceinline__ void sb_average(const float2 *X, double *ma, double *maa, double *peak, double *s_red, SpecBankTrk &t, int Fi, double rate,
                                           int do_peak) {
    const int F = Fi >> 1, tid = threadIdx.x;
    double mx = 0.0, mn = 1.0;
    for (int x = tid; x < F; x += kFftThreads) {
        const int k = (2 * x + F) & (Fi - 1);
        const float2 va = X[k], vb = X[k + 1];
        const float ra = sqrtf(rounded(va.x * va.x) + rounded(va.y * va.y));
        const float rb = sqrtf(rounded(vb.x * vb.x) + rounded(vb.y * vb.y));
        AvgState s;
        s.ma_a = ma[2 * x]; s.ma_b = ma[2 * x + 1]; s.maa_a = maa[2 * x]; s.maa_b = maa[2 * x + 1];
        avg_step(s, (double)ra, (double)rb, rate);
        ma[2 * x] = s.ma_a; ma[2 * x + 1] = s.ma_b; maa[2 * x] = s.maa_a; maa[2 * x + 1] = s.maa_b;
        // (fft_ceil / fft_floor are floats that take a value only through `>` / `<`: they never turn NaN, so the `!=` halves of :500 / :503 never
        //  fire, and a NaN bin never wins: fmax / fmin pass it over.  The float rounding commutes with the maximum: applied once, below.)
        mx = fmax(mx, fmax(s.maa_a, s.maa_b)); mn = fmin(mn, fmin(s.maa_a, s.maa_b));
        if (do_peak) {
            if (s.maa_a > peak[2 * x]) peak[2 * x] = s.maa_a;
            if (s.maa_b > peak[2 * x + 1]) peak[2 * x + 1] = s.maa_b;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { mx = fmax(mx, __shfl_down(mx, o, 64)); mn = fmin(mn, __shfl_down(mn, o, 64)); }
    if ((tid & 63) == 0) { s_red[tid >> 6] = mx; s_red[4 + (tid >> 6)] = mn; }
    __syncthreads();                                                        // (also: every thread's maa[] / peak[] store is visible to the workgroup)
    const float fft_ceil = (float)fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
    const float fft_floor = (float)fmin(fmin(s_red[4], s_red[5]), fmin(s_red[6], s_red[7]));
    if (t.ceil_ma != t.ceil_ma) t.ceil_ma = fft_ceil;                       // :513-521
    t.ceil_ma = t.ceil_ma + ((double)fft_ceil - t.ceil_ma) * 0.05;
    if (t.ceil_maa != t.ceil_maa) t.ceil_maa = fft_ceil;
    t.ceil_maa = t.ceil_maa + (t.ceil_ma - t.ceil_maa) * 0.05;
    if (t.floor_ma != t.floor_ma) t.floor_ma = fft_floor;
    t.floor_ma = t.floor_ma + ((double)fft_floor - t.floor_ma) * 0.05;
    if (t.floor_maa != t.floor_maa) t.floor_maa = fft_floor;
    t.floor_maa = t.floor_maa + (t.floor_ma - t.floor_maa) * 0.05;
    if (do_peak) {                                                          // :523-530
        if (t.ceil_maa > t.ceil_peak) t.ceil_peak = t.ceil_maa;
        if (t.floor_maa < t.floor_peak) t.floor_peak = t.floor_maa;
    }
}

// the display's scale (:539-540), one display point from the sum of its `bins` averager values (:562-576), and what csdr_*_fetch reads of a frame
struct SpecBankScale { double pc, pf, den; };
__device__ __forceinline__ SpecBankScale sb_scale(const SpecBankTrk &t, int do_peak) {
    SpecBankScale sc;
    sc.pc = do_peak ? t.ceil_peak : t.ceil_maa; sc.pf = do_peak ? t.floor_peak : t.floor_maa;
    sc.den = log10((sc.pc + 0.25) - (sc.pf - 0.75));
    return sc;
}
__device__ __forceinline__ float sb_point(double acc, double bins, const SpecBankScale &sc, float sf) {
    return (float)((log10((acc / bins) + 0.25 - (sc.pf - 0.75)) / sc.den) * (double)sf);
}
__device__ __forceinline__ void sb_store_meta(SpecBankFrame *meta, const SpecBankScale &sc, int do_peak) {
    if (threadIdx.x == 0) {
        SpecBankFrame m;
        m.point_ceil = sc.pc; m.point_floor = sc.pf; m.hold = do_peak; m.pad = 0;
        *meta = m;
    }
}

CSDR_KERNEL_SB __launch_bounds__(kFftThreads) void specbank_process(SpecBankArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Fi = a.Fi, F = Fi >> 1, tid = threadIdx.x;
    float2 *sa = reinterpret_cast<float2 *>(smem), *sb = sa + Fi;
    double *s_red = reinterpret_cast<double *>(sb + Fi);                   // [2][4 waves]
    const SpecBankRun run = a.runs[blockIdx.x];
    const size_t so = (size_t)run.slot * Fi;
    float2 *last = a.last + so;
    double *ma = a.ma + so, *maa = a.maa + so, *peak = a.peak + so;
    SpecBankTrk t = a.trk[run.slot];                                       // every thread carries the trackers
    for (int jn = 0; jn < run.n_jobs; ++jn) {
        const SpecBankJob jb = a.jobs[run.job0 + jn];
        if (jb.peak_reset_now) sb_peak_reset(peak, t, Fi);
        if (jb.action == kSbPrime) { sb_prime(last, jb.src, jb.n, jb.arg); continue; }
        const float2 *X = sb_transform(last, jb.src, jb.n, jb.arg, Fi, sa, sb, a.tw4096);
        sb_average(X, ma, maa, peak, s_red, t, Fi, a.rate, jb.do_peak);
        const SpecBankScale sc = sb_scale(t, jb.do_peak);
        const size_t fo = (size_t)run.slot * a.max_frames + (size_t)jb.frame;
        float *out = a.points + fo * F, *hold = a.hold + fo * F;
        for (int x = tid; x < F; x += kFftThreads) {                        // :542-576: bins 2x, 2x + 1; idx == 0 is replaced by fft_floor_maa
            out[x] = sb_point((x == 0 ? t.floor_maa : maa[2 * x]) + maa[2 * x + 1], 2.0, sc, a.sf);
            if (jb.do_peak) hold[x] = sb_point((x == 0 ? t.floor_maa : peak[2 * x]) + peak[2 * x + 1], 2.0, sc, a.sf);
        }
        sb_store_meta(a.meta + fo, sc, jb.do_peak);
        __syncthreads();                                                    // the LDS arrays and `last` are reused by the next job
    }
    if (tid == 0) a.trk[run.slot] = t;
}

}  // namespace csdr
