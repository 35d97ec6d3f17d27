// kernels_scopebank.hpp -- N independent ScopeVisualProcessors in two launches (csdr_scopebank, include/csdr_hip.h "Scope bank").
//
// Replaces, per slot and per process() input (reference file:line, src/process/ScopeVisualProcessor.cpp):
//   waveform normalisation in the modes Y / 2Y / XY                :64-117    (scopebank_wave)
//   the zero-padded real input, stereo as left + right             :119-141   (scopebank_spectrum, as all below)
//   fft_execute                                                    :163       (lds_fft of kernels_spec.hpp, fftSize <= 4096 points in LDS)
//   double magnitude, the two double averagers                     :165-177
//   double extrema, the four trackers at 0.05                      :179-190
//   log10 scaling of outSize points                                :194-214   (outSize itself: the host, by the float arithmetic of :194-200)
// The per-frame statements are scope_wave_frame / scope_spectrum_frame of kernels_io.hpp, the ones csdr_scope's kernels run: a slot's items are a
// csdr_scope's bit for bit.  The waveform carries no state: one workgroup per (slot, frame) job.  The spectrum's averagers and trackers are
// recurrences over a slot's frames and slots share nothing: one workgroup per slot walks that slot's job records in order.  That kernel is
// latency-bound (the chain of radix passes with their barriers, as specbank_process is); the parallelism is across slots.
// All LDS is dynamic (`smem`): scopebank_wave four floats; scopebank_spectrum 2 * L float2 (ping-pong of the transform) + 8 doubles of reduction scratch.
#pragma once
#include "common.hpp"
#include "stream_order.hpp"
#include "kernels_io.hpp"

#if defined(CSDR_TU_SCOPEBANK)
#define CSDR_KERNEL_SCB CSDR_KERNEL
#else
#define CSDR_KERNEL_SCB CSDR_KERNEL_ELSEWHERE
#endif

namespace csdr {

struct ScopeBankJob {            // one non-empty process() input of a slot
    ScopeFrame fr;
    int32_t slot;
    int32_t frame;               // output frame of the slot in this call
};
static_assert(sizeof(ScopeFrame) == 56 && sizeof(ScopeBankJob) == 64, "ScopeBankJob layout");
using ScopeBankRun = SlotRun;                                            // one workgroup of scopebank_spectrum: jobs [job0, job0 + n_jobs) of `slot`

struct ScopeBankArgs {
    const ScopeBankRun *runs;
    const ScopeBankJob *jobs;
    const float2 *tw4096;
    double *ma, *maa;            // [slots][L / 2]
    ScopeTrk *trk;               // [slots]
    float *wave_pts;             // [slots][max_frames][2 * max_n]
    float *spec_pts;             // [slots][max_frames][L]
    ScopeMeta *wave_meta, *spec_meta;    // [slots][max_frames]
    int32_t L, max_frames, max_n, max_scope_samples;
    double rate;                 // fft_average_rate (a float member: the host widens it)
};

__host__ __device__ constexpr size_t scopebank_lds_bytes(int L) { return (size_t)2 * L * sizeof(float2) + 8 * sizeof(double); }

// ---- waveform.  grid = the jobs of the call
CSDR_KERNEL_SCB __launch_bounds__(kScopeThreads) void scopebank_wave(ScopeBankArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ScopeBankJob *jb = a.jobs + blockIdx.x;
    const ScopeFrame fr = scope_load(&jb->fr, 0);
    const size_t fo = (size_t)jb->slot * a.max_frames + (size_t)jb->frame;
    scope_wave_frame(fr, a.max_scope_samples, a.wave_pts + fo * 2 * (size_t)a.max_n, a.wave_meta + fo, reinterpret_cast<float *>(smem));
}

// ---- audio spectrum.  grid = the slots that have jobs
CSDR_KERNEL_SCB __launch_bounds__(kFftThreads) void scopebank_spectrum(ScopeBankArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int L = a.L;
    float2 *sa = reinterpret_cast<float2 *>(smem), *sb = sa + L;
    double *s_red = reinterpret_cast<double *>(sb + L);                    // [2][4 waves]
    const ScopeBankRun run = a.runs[blockIdx.x];
    const size_t so = (size_t)run.slot * (size_t)(L >> 1);
    double *ma = a.ma + so, *maa = a.maa + so;
    ScopeTrk t = a.trk[run.slot];                                          // every thread carries the trackers
    for (int jn = 0; jn < run.n_jobs; ++jn) {
        const ScopeBankJob *jb = a.jobs + run.job0 + jn;
        const ScopeFrame fr = scope_load(&jb->fr, 0);
        const size_t fo = (size_t)run.slot * a.max_frames + (size_t)jb->frame;
        scope_spectrum_frame(fr, L, a.rate, a.tw4096, ma, maa, t, a.spec_pts + fo * (size_t)L, a.spec_meta + fo, sa, sb, s_red);
    }
    if (threadIdx.x == 0) a.trk[run.slot] = t;
}

}  // namespace csdr
