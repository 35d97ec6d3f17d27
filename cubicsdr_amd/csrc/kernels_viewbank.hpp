// kernels_viewbank.hpp -- N independent SpectrumVisualProcessors in ZOOMED view in one launch (csdr_viewbank, include/csdr_hip.h "View bank").
//
// Replaces, per slot and per process() input (reference file:line, src/process/SpectrumVisualProcessor.cpp):
//   the reset of fft_result_peak / fft_ceil_peak / fft_floor_peak  :264-273   (which input it falls in front of: the host's countdown)
//   the move of fft_result_ma / _maa on a retune                    :316-331   (whether, which way and how far: the host, from the frequencies alone)
//   nco_crcf_mix_block_up / _down                                   :341-352   (table NCO, the phase word carried by the host)
//   msresamp_crcf_execute                                           :379       (half-band decimators + arbitrary polyphase stage; the counts: the host)
//   frame selection                                                 :387-421   (which branch: the host, from num_written alone; the copies: here)
//   fft_execute, float magnitude with the half swap                 :439-452
//   the stretch / squeeze of the averagers behind a new resampler   :454-492
//   NaN re-seeding, the two double averagers, ceiling / floor       :494-505
//   running peak, the four trackers at 0.05                         :506-530
//   display points over the view's bin walk, hold points            :532-576, :626-627  (the walk's map: the host, per (bandwidth, resampleBw))
//   hideDC                                                          :578-623   (a gather: the sources lie outside the span)
// One workgroup per slot walks that slot's job records in order, as specbank_process does: averagers, trackers and the resampler's windows are
// recurrences over a slot's inputs, and slots share nothing.  Per job two phases share the LDS:
//   A  the first `n` samples are mixed and run through the cascade in chunks of kFeChunk stream samples, with the demodulator front-end's LDS layout
//      and stage arithmetic (fe_stage_any, the 14-tap arms in tap order).  Here ONE workgroup owns the whole stream of its slot, so the windows are
//      carried as state: per stage the last kFeTail even / odd samples, the last kFeZTail chain outputs, and the mixed samples that do not yet fill a
//      group of 2^S (msresamp's buffer_index).  Every output is one dot product over positions of the slot's stream: bit for bit the same however
//      the inputs are cut into calls.  The first Fi outputs go to the slot's `y` row in HBM.
//   B  the per-frame functions of kernels_specbank.hpp (sb_prime, sb_transform, sb_average, sb_scale, sb_point, sb_store_meta: ONE statement for
//      both banks) on that row, with the averagers' moves staged through LDS in front of them (every kept value is read before any is written).
//      What is stated here is what differs: the point loop walks the view map and gathers through the hideDC span.
// The kernel is latency-bound by design, as specbank_process is.  All LDS is dynamic (`smem`): the larger of the two phases' needs.
#pragma once
#include "common.hpp"
#include "kernels_spec.hpp"
#include "kernels_demod.hpp"
#include "kernels_waterfall.hpp"
#include "kernels_specbank.hpp"

#if defined(CSDR_TU_VIEWBANK)
#define CSDR_KERNEL_VB CSDR_KERNEL
#else
#define CSDR_KERNEL_VB CSDR_KERNEL_ELSEWHERE
#endif

namespace csdr {

constexpr int kVbNone = 3;                                   // action: the input ended at :284-287 (sample_rate 0)
constexpr int kVbLeft = 1, kVbRight = 2, kVbSqueeze = 3, kVbStretch = 4;     // moves of the averagers
constexpr int kVbPendMax = 1 << kMaxHb;                      // mixed samples in front of a whole group of 2^S
constexpr int kVbTailLen = kMaxHb * 2 * kFeTail;             // [stage][even | odd][kFeTail]
constexpr int kVbState = kVbPendMax + kVbTailLen + kFeZTail; // float2 of resampler state per slot

struct ViewBankJob {             // one non-empty process() input of a slot
    const float2 *src;           // the input's samples (device memory)
    const int2 *map;             // (first bin, bins) of every display point for this input's (bandwidth, resampleBw)
    int32_t n;                   // samples consumed: min(input length, desiredInputSize) (:295-302)
    int32_t cfg;                 // the resampler in force: index into ViewBankArgs::cfgs / ::arms
    uint32_t theta0, dtheta;     // oscillator phase word in front of the input, increment
    int32_t mixdir;              // 0: centerFreq == frequency (:351); +1: up; -1: down (:345-349)
    int32_t buf0;                // mixed samples waiting in front of the input (buffer_index)
    uint32_t phase0;             // arbitrary stage's phase in front of the input
    int32_t rebuild;             // a new resampler (:354-368): every window empty
    int32_t nw;                  // num_written
    int32_t shift_mode, shift_n; // retune (:316-331): kVbLeft / kVbRight by shift_n bins; 0: none
    int32_t rescale;             // kVbSqueeze / kVbStretch in front of this frame's averaging (:454-492); 0: none
    int32_t action;              // kSbPrime | kSbSlide | kSbFull on num_written | kVbNone
    int32_t arg;                 // as SpecBankJob::arg
    int32_t frame;               // output frame of the slot in this call; -1: none
    int32_t do_peak;             // doPeak of this input (:247)
    int32_t peak_reset_now;      // peakReset reached 0 in front of this input (:264-273)
    int32_t dc_start, dc_half, dc_end;      // hideDC span of this frame (HideDcSpan; empty: off or out of view)
};
static_assert(sizeof(ViewBankJob) == 96, "ViewBankJob layout");

struct ViewBankArgs {
    const SpecBankRun *runs;
    const ViewBankJob *jobs;
    const float2 *tw4096;
    const float *sintab;         // the NCO's 1024-entry table
    const ResampCfg *cfgs;       // the resamplers the object has designed so far
    const float *arms;           // [cfg][kArms][kArmTaps]
    float2 *last;                // [slots][Fi]  fftLastData
    double *ma, *maa, *peak;     // [slots][Fi]
    SpecBankTrk *trk;            // [slots]
    float2 *rs;                  // [slots][kVbState]  pending mixed samples | stage tails | chain-output tail
    float2 *y;                   // [slots][Fi]  the resampler's output of the input being processed
    float *points, *hold;        // [slots][max_frames][F]
    SpecBankFrame *meta;         // [slots][max_frames]
    int32_t Fi, max_frames;
    double rate;
    float sf;
};

__host__ __device__ inline size_t viewbank_lds_bytes(int Fi, int S_max) {
    return specbank_lds_bytes(Fi) > fe_lds_bytes(S_max) ? specbank_lds_bytes(Fi) : fe_lds_bytes(S_max);
}

__device__ inline float2 vb_mix(float2 x, int rel, const ViewBankJob &jb, const float *tab) {
    if (jb.mixdir == 0) return x;
    float s, c;
    nco_sincos(tab, jb.theta0 + (uint32_t)rel * jb.dtheta, s, c);
    if (jb.mixdir < 0) return make_float2(fmaf(x.x, c, x.y * s), fmaf(x.y, c, -x.x * s));    // x (c - j s)
    return make_float2(fmaf(x.x, c, -x.y * s), fmaf(x.y, c, x.x * s));                         // x (c + j s)
}

// one move of an averager array, staged through LDS
__device__ inline void vb_move(double *v, int mode, int n, int Fi, double *stage) {
    const int tid = threadIdx.x;
    for (int i = tid; i < Fi; i += kFftThreads) stage[i] = v[i];
    __syncthreads();
    if (mode == kVbLeft) { for (int i = tid; i < Fi - n; i += kFftThreads) v[i] = stage[i + n]; }                 // memmove :323-324
    else if (mode == kVbRight) { for (int i = tid; i < Fi - n; i += kFftThreads) v[i + n] = stage[i]; }           // memmove :328-329
    else if (mode == kVbSqueeze) { for (int i = tid; i < Fi; i += kFftThreads) v[i] = stage[Fi / 4 + i / 2]; }
    else for (int i = tid; i < Fi; i += kFftThreads) v[i] = (i >= Fi / 4 && i < Fi - Fi / 4) ? stage[(i - Fi / 4) * 2] : 0.0;
    __syncthreads();
}

// phase A: the stream of the slot is (pending mixed samples) ++ (the input, mixed); whole groups of 2^S run through the cascade
__device__ inline void vb_resample(const ViewBankJob &jb, const ResampCfg &cfg, const float *__restrict__ arms, const float *__restrict__ sintab,
                                   float2 *pend, float2 *tails, float2 *ztail, float2 *y, int Fi, char *smem) {
    const int tid = threadIdx.x;
    const int S = cfg.S;
    const uint32_t step = cfg.step;
    const int alen = fe_arr_len(S);
    float2 *LE = reinterpret_cast<float2 *>(smem);
    float2 *LO = LE + alen;
    float2 *LZ = LO + alen;
    float *tab = reinterpret_cast<float *>(LZ + fe_z_len(S));
    float *hb = tab + 1024;
    for (int i = tid; i < 1024; i += kFftThreads) tab[i] = sintab[i];
    for (int i = tid; i < S * kHbMaxM; i += kFftThreads) hb[i] = cfg.h_x[i / kHbMaxM][i % kHbMaxM];
    for (int i = tid; i < S * kFeTail; i += kFftThreads) {
        const int e = i / kFeTail, k = i % kFeTail;
        LE[fe_off(e) + k] = jb.rebuild ? make_float2(0.f, 0.f) : tails[(2 * e) * kFeTail + k];
        LO[fe_off(e) + k] = jb.rebuild ? make_float2(0.f, 0.f) : tails[(2 * e + 1) * kFeTail + k];
    }
    if (tid < kFeZTail) LZ[tid] = jb.rebuild ? make_float2(0.f, 0.f) : ztail[tid];
    const int total = jb.buf0 + jb.n;
    const int u_stop = (total >> S) << S;
    const float zeta = 1.0f / (float)(1 << S);
    __syncthreads();
    for (int uc = 0; uc < u_stop; uc += kFeChunk) {
        const int n = min(kFeChunk, u_stop - uc);
        for (int p = tid; 2 * p < n; p += kFftThreads) {
            const int u = uc + 2 * p;
            const float2 va = u < jb.buf0 ? pend[u] : vb_mix(jb.src[u - jb.buf0], u - jb.buf0, jb, tab);
            float2 vb = make_float2(0.f, 0.f);
            if (2 * p + 1 < n) vb = u + 1 < jb.buf0 ? pend[u + 1] : vb_mix(jb.src[u + 1 - jb.buf0], u + 1 - jb.buf0, jb, tab);
            if (S == 0) { LZ[kFeZTail + 2 * p] = va; if (2 * p + 1 < n) LZ[kFeZTail + 2 * p + 1] = vb; }
            else { LE[kFeTail + p] = va; LO[kFeTail + p] = vb; }
        }
        __syncthreads();
        int cnt = n;
        for (int e = 0; e < S; ++e) {
            cnt >>= 1;
            const float2 *Ein = LE + fe_off(e) + kFeTail, *Oin = LO + fe_off(e) + kFeTail;
            const bool tz = (e == S - 1);
            float2 *oE = LE + (tz ? 0 : fe_off(e + 1) + kFeTail), *oO = LO + (tz ? 0 : fe_off(e + 1) + kFeTail), *oZ = LZ + kFeZTail;
            fe_stage_any(cfg.m_x[e], Ein, Oin, hb + e * kHbMaxM, cnt, zeta, tz, oE, oO, oZ);
            __syncthreads();
        }
        // arbitrary stage: the outputs whose newest chain sample lies in this chunk
        const int64_t kz0 = uc >> S;
        const int cz = n >> S;
        const int64_t ja = resamp_first_out(kz0, jb.phase0, step), je = resamp_first_out(kz0 + cz, jb.phase0, step);
        for (int64_t j = ja + tid; j < je && j < Fi; j += kFftThreads) {
            const int64_t Pj = (int64_t)jb.phase0 + j * (int64_t)step;
            const int kq = (int)((Pj >> 24) - kz0);
            const float *h = arms + (int)((Pj & 0xFFFFFF) >> 16) * kArmTaps;
            const float2 *z = LZ + kFeZTail + kq - (kArmTaps - 1);
            float ar = 0.f, ai = 0.f;
            for (int t = 0; t < kArmTaps; ++t) { ar = fmaf(h[t], z[t].x, ar); ai = fmaf(h[t], z[t].y, ai); }
            y[j] = make_float2(ar, ai);
        }
        // the tails move to the front of every array (read, barrier, write: the writes touch tail entries only)
        float2 cv[2];
        const int ntail = 2 * kFeTail * S;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int idx = tid + r * kFftThreads;
            if (idx < ntail) {
                const int e = idx / (2 * kFeTail), k = idx % (2 * kFeTail);
                const float2 *arr = k < kFeTail ? LE : LO;
                cv[r] = arr[fe_off(e) + (n >> (e + 1)) + (k % kFeTail)];
            }
        }
        float2 vz = make_float2(0.f, 0.f);
        if (tid < kFeZTail) vz = LZ[cz + tid];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int idx = tid + r * kFftThreads;
            if (idx < ntail) {
                const int e = idx / (2 * kFeTail), k = idx % (2 * kFeTail);
                float2 *arr = k < kFeTail ? LE : LO;
                arr[fe_off(e) + (k % kFeTail)] = cv[r];
            }
        }
        if (tid < kFeZTail) LZ[tid] = vz;
    }
    __syncthreads();
    for (int i = tid; i < S * kFeTail; i += kFftThreads) {
        const int e = i / kFeTail, k = i % kFeTail;
        tails[(2 * e) * kFeTail + k] = LE[fe_off(e) + k];
        tails[(2 * e + 1) * kFeTail + k] = LO[fe_off(e) + k];
    }
    if (tid < kFeZTail) ztail[tid] = LZ[tid];
    // what does not fill a group waits (mixed) for the next input; with u_stop > 0 all of it comes from this input (buf0 < 2^S <= u_stop)
    if (u_stop == 0) { for (int i = jb.buf0 + tid; i < total; i += kFftThreads) pend[i] = vb_mix(jb.src[i - jb.buf0], i - jb.buf0, jb, tab); }
    else for (int i = tid; i < total - u_stop; i += kFftThreads) pend[i] = vb_mix(jb.src[u_stop + i - jb.buf0], u_stop + i - jb.buf0, jb, tab);
    __syncthreads();                                                       // `y` and the state are read across threads; the LDS is phase B's now
}

CSDR_KERNEL_VB __launch_bounds__(kFftThreads) void viewbank_process(ViewBankArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Fi = a.Fi, F = Fi >> 1, tid = threadIdx.x;
    float2 *sa = reinterpret_cast<float2 *>(smem), *sb = sa + Fi;
    double *s_red = reinterpret_cast<double *>(sb + Fi);                   // [2][4 waves]
    double *s_stage = reinterpret_cast<double *>(smem);                    // [Fi]: an averager array on its move
    const SpecBankRun run = a.runs[blockIdx.x];
    const size_t so = (size_t)run.slot * Fi;
    float2 *last = a.last + so, *y = a.y + so;
    double *ma = a.ma + so, *maa = a.maa + so, *peak = a.peak + so;
    float2 *pend = a.rs + (size_t)run.slot * kVbState, *tails = pend + kVbPendMax, *ztail = tails + kVbTailLen;
    SpecBankTrk t = a.trk[run.slot];                                       // every thread carries the trackers
    for (int jn = 0; jn < run.n_jobs; ++jn) {
        const ViewBankJob jb = a.jobs[run.job0 + jn];
        if (jb.peak_reset_now) sb_peak_reset(peak, t, Fi);
        if (jb.action == kVbNone) { __syncthreads(); continue; }           // :284-287
        if (jb.shift_mode) {                                               // :316-331 (the peak array stays)
            vb_move(ma, jb.shift_mode, jb.shift_n, Fi, s_stage);
            vb_move(maa, jb.shift_mode, jb.shift_n, Fi, s_stage);
        }
        vb_resample(jb, a.cfgs[jb.cfg], a.arms + (size_t)jb.cfg * kArms * kArmTaps, a.sintab, pend, tails, ztail, y, Fi, smem);
        const int nw = min(jb.nw, Fi);                                     // fftInData holds Fi samples (:388-396)
        if (jb.action == kSbPrime) { sb_prime(last, y, nw, jb.arg); continue; }
        if (jb.rescale) {                                                  // :454-492
            vb_move(ma, jb.rescale, 0, Fi, s_stage);
            vb_move(maa, jb.rescale, 0, Fi, s_stage);
        }
        const float2 *X = sb_transform(last, y, nw, jb.arg, Fi, sa, sb, a.tw4096);
        sb_average(X, ma, maa, peak, s_red, t, Fi, a.rate, jb.do_peak);
        const SpecBankScale sc = sb_scale(t, jb.do_peak);
        const size_t fo = (size_t)run.slot * a.max_frames + (size_t)jb.frame;
        float *out = a.points + fo * F, *hold = a.hold + fo * F;
        HideDcSpan dc;
        dc.start = jb.dc_start; dc.half = jb.dc_half; dc.end = jb.dc_end;
        for (int x = tid; x < F; x += kFftThreads) {                        // :542-576 over the view's walk; a point inside the hideDC span shows its mirror's value
            const int2 m = jb.map[hide_dc_source(dc, x)];
            double acc = 0.0, pacc = 0.0;
            for (int c = 0; c < m.y; ++c) {
                const int idx = m.x + c;
                const bool in = idx > 0 && idx < Fi;                        // :546-551
                acc += in ? maa[idx] : t.floor_maa;
                if (jb.do_peak) pacc += in ? peak[idx] : t.floor_maa;
            }
            out[x] = sb_point(acc, (double)m.y, sc, a.sf);
            if (jb.do_peak) hold[x] = sb_point(pacc, (double)m.y, sc, a.sf);
        }
        sb_store_meta(a.meta + fo, sc, jb.do_peak);
        __syncthreads();                                                    // the LDS arrays, `last` and the averagers are reused by the next job
    }
    if (tid == 0) a.trk[run.slot] = t;
}

}  // namespace csdr
