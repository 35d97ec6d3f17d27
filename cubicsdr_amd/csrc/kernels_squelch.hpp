// kernels_squelch.hpp -- the level gate of N demodulators in three launches (csdr_squelch, include/csdr_hip.h "Squelch bank").
//
// Replaces, per slot and per block (reference file:line):
//   linearToDb, currentSignalLevel                              src/demod/DemodulatorThread.cpp:59-67, :142-165   (squelch_scan, lanes)
//   signalFloor / signalCeil, signalLevel, squelched            :167-198                                          (squelch_scan, the walk)
//   squelchBreak                                                :200-220
//   the condition of the audio push                             :318-328    (flag bit 2)
//   the recorder's squelch options                              src/audio/AudioSinkFileThread.cpp:27-44           (the walk's offsets, squelch_pcm16)
//   AudioFileWAV's payload conversion                           src/audio/AudioFileWAV.cpp:133-157                (squelch_pcm16: pcm16_scale / pcm16_sample of kernels_io.hpp)
// The trackers are a recurrence over a slot's blocks and slots share nothing: one 64-lane wave per slot, four slots per workgroup.  The one expensive
// operation of a block is the double log10, and it does not depend on the state: the lanes take 64 blocks at a time, one each, and leave the dB value
// and the block's sampleTime in LDS; lane 0 then carries the state over them and leaves the items in LDS, and the lanes store them.  The waves of a
// workgroup never meet: every hand-off is wave-local (wave_sync).  The recurrence is compiled with contraction off, so log10 is the only operation
// whose result can differ from the host's (host/DemodLevel.h states the same arithmetic for one block).
// All LDS is dynamic (`smem`): squelch_scan kSqWaves * sizeof(SquelchLds); squelch_pack 256 int64; squelch_pcm16 none.
#pragma once
#include "common.hpp"
#include "kernels_demod.hpp"
#include "kernels_io.hpp"

#if defined(CSDR_TU_SQUELCH)
#define CSDR_KERNEL_SQ CSDR_KERNEL
#else
#define CSDR_KERNEL_SQ CSDR_KERNEL_ELSEWHERE
#endif

namespace csdr {

constexpr int kSqWaves = 4;                  // slots per workgroup of squelch_scan
constexpr int kSqMaxSlots = 4096;            // squelch_pack: one workgroup of 256 threads, at most 16 slots each

struct SquelchState { float level, floor, ceil; int32_t brk; };       // signalLevel, signalFloor, signalCeil, squelchBreak
struct SquelchRec { int32_t src_off, n, dst_off; float peak; };       // one block for the recorder: floats at src_off of the slot's audio; n < 0: -n zeros;
                                                                      // dst_off < 0: left out; dst_off counts from the slot's base in the packed stream
static_assert(sizeof(csdr_squelch_item) == 16 && sizeof(SquelchState) == 16 && sizeof(SquelchRec) == 16, "squelch record layouts");

struct SquelchRun {                          // one stepped slot of a call
    int32_t slot, n_blocks;
    int32_t enabled, muted, record;          // the settings in force for this call
    float level_db;
    int32_t sample_rate;
    int32_t ash;                             // bank form: floats per audio-arbitrary output = 2^ash; -1: no audio stage (digital slots: n_audio = 0)
    const csdr_squelch_block *blocks;        // explicit form: [n_blocks]; nullptr: the bank form
    const BlockOut *bout;                    // bank form: the slot's level sums and peaks where the audio kernels left them
    const BlockPlan *plan;                   // bank form: the slot's block starts, [n_blocks + 1]
    const float *audio;                      // the slot's audio (explicit form: the blocks back to back); nullptr: nothing to record
};
static_assert(sizeof(SquelchRun) == 64, "SquelchRun layout");

struct SquelchArgs {
    const SquelchRun *runs;
    int32_t n_runs, max_blocks;
    SquelchState *state;                     // [slots]
    csdr_squelch_item *items;                // [slots][max_blocks]
    uint8_t *flags;                          // [slots][max_blocks]
    SquelchRec *recs;                        // [slots][max_blocks]
    int32_t *totals;                         // [slots] floats the slot records in this call
    const int64_t *pack;                     // [slots + 1] exclusive scan of totals (squelch_pack)
    int16_t *pcm;
};

struct SquelchLds {                          // of one wave: a chunk of 64 blocks
    double db[64], sample_time[64];
    int32_t n_audio[64], src_off[64];
    float peak[64];
    csdr_squelch_item item[64];
    SquelchRec rec[64];
};

// one block of DemodulatorThread::run's level bookkeeping (:142-220), the statements of host/DemodLevel.h in the same types: float trackers, the
// updates in double, stored as float.  Returns the item's flags.
__device__ inline uint32_t squelch_step(SquelchState &s, bool have_level, double level_db, double sampleTime, bool squelchEnabled, float squelchLevel, bool muted) {
#pragma clang fp contract(off)
    double currentSignalLevel = 0;
    if (have_level) {
        currentSignalLevel = level_db;
        float sf = s.floor, sc = s.ceil, sl = squelchLevel;
        if (currentSignalLevel > sc) sc = (float)currentSignalLevel;
        if (currentSignalLevel < sf) sf = (float)currentSignalLevel;
        if (sl + 1.0f > sc) sc = sl + 1.0f;
        if ((sf + 2.0f) > sc) sc = sf + 2.0f;
        sc -= (sc - (currentSignalLevel + 2.0f)) * sampleTime * 0.05f;
        sf += ((currentSignalLevel - 5.0f) - sf) * sampleTime * 0.15f;
        s.floor = sf; s.ceil = sc;
    }
    float lvl = s.level;
    if (currentSignalLevel > lvl) lvl = lvl + (currentSignalLevel - lvl) * 0.5;
    else lvl = lvl + (currentSignalLevel - lvl) * 0.05 * sampleTime * 30.0;
    s.level = lvl;
    const bool squelched = squelchEnabled && (lvl < squelchLevel);                      // :198
    if (squelchEnabled) {                                                              // :200-220 (the solo-mode lock is GUI state)
        if (!squelched && !s.brk) s.brk = 1;
        else if (squelched && s.brk) s.brk = 0;
    }
    return (squelched ? 1u : 0u) | (s.brk ? 2u : 0u) | ((!squelched && !muted) ? 4u : 0u);     // bit 2: the audio push of :318-328
}

// ---- the level gate.  grid = ceil(runs / kSqWaves), kSqWaves * 64 threads
CSDR_KERNEL_SQ __launch_bounds__(kSqWaves * 64) void squelch_scan(SquelchArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.x * kSqWaves + wave;
    if (r >= a.n_runs) return;                                                         // (a whole wave: the waves of a workgroup share no barrier)
    SquelchLds &L = reinterpret_cast<SquelchLds *>(smem)[wave];
    const SquelchRun run = a.runs[r];
    const size_t row = (size_t)run.slot * (size_t)a.max_blocks;
    SquelchState st = a.state[run.slot];                                               // lane 0 carries it
    int32_t src_at = 0, dst_at = 0;
    for (int b0 = 0; b0 < run.n_blocks; b0 += 64) {
        const int nb = min(64, run.n_blocks - b0), b = b0 + lane;
        if (lane < nb) {
            double accum = 0.0;
            int32_t count = 0, n_in, n_audio, src = -1;
            float peak = 0.0f;
            if (run.blocks) {
                const csdr_squelch_block blk = run.blocks[b];
                accum = blk.level_accum; count = blk.level_count; n_in = blk.n_in; n_audio = blk.n_audio; peak = blk.audio_peak;
            } else {
                const BlockPlan p0 = run.plan[b], p1 = run.plan[b + 1];
                n_in = p1.j0 - p0.j0;
                n_audio = run.ash < 0 ? 0 : (p1.q0 - p0.q0) << run.ash;
                src = run.ash < 0 ? 0 : p0.q0 << run.ash;
                if (n_audio > 0) { const BlockOut o = run.bout[b]; accum = o.level_accum; count = o.level_count; peak = o.audio_peak; }
            }
            double db = 0.0;
            if (n_audio > 0) {                                                         // linearToDb :59-67
                double linear = accum / (double)count;
                if (linear <= 1e-20) linear = 1e-20;
                db = 20.0 * log10(linear);
            }
            L.db[lane] = db;
            L.sample_time[lane] = (double)n_in / (double)run.sample_rate;
            L.n_audio[lane] = n_audio; L.src_off[lane] = src; L.peak[lane] = peak;
        }
        wave_sync();
        if (lane == 0) {
            for (int k = 0; k < nb; ++k) {
                const int32_t n_audio = L.n_audio[k];
                const uint32_t fl = squelch_step(st, n_audio > 0, L.db[k], L.sample_time[k], run.enabled != 0, run.level_db, run.muted != 0);
                csdr_squelch_item it;
                it.level = st.level; it.floor = st.floor; it.ceil = st.ceil; it.flags = fl;
                L.item[k] = it;
                // AudioSinkFileThread.cpp:27-44: squelched blocks as zeros, left out, or as if there were no squelch
                const bool squelched = (fl & 1u) != 0;
                const bool keep = run.audio != nullptr && n_audio > 0 && (!squelched || run.record != 1);
                SquelchRec rc;
                rc.src_off = run.blocks ? src_at : L.src_off[k];
                rc.n = (squelched && run.record == 0) ? -n_audio : n_audio;
                rc.dst_off = keep ? dst_at : -1;
                rc.peak = L.peak[k];
                L.rec[k] = rc;
                src_at += n_audio;
                if (keep) dst_at += n_audio;
            }
        }
        wave_sync();
        if (lane < nb) {
            a.items[row + b] = L.item[lane];
            a.flags[row + b] = (uint8_t)L.item[lane].flags;
            a.recs[row + b] = L.rec[lane];
        }
        wave_sync();                                                                   // (the next chunk rewrites the arrays)
    }
    if (lane == 0) { a.state[run.slot] = st; a.totals[run.slot] = dst_at; }
}

// ---- the slots' bases in the packed recorder stream: an exclusive scan of the totals.  ONE workgroup of 256 threads, each with a run of at most
// kSqMaxSlots / 256 consecutive slots
CSDR_KERNEL_SQ __launch_bounds__(256) void squelch_pack(const int32_t *__restrict__ totals, int64_t *__restrict__ pack, int n_slots) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int64_t *part = reinterpret_cast<int64_t *>(smem);                                 // [256]
    const int t = (int)threadIdx.x, per = (n_slots + 255) / 256, s0 = min(n_slots, t * per), s1 = min(n_slots, s0 + per);
    int64_t sum = 0;
    for (int s = s0; s < s1; ++s) sum += totals[s];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t at = 0;
        for (int i = 0; i < 256; ++i) { const int64_t v = part[i]; part[i] = at; at += v; }
        pack[n_slots] = at;
    }
    __syncthreads();
    int64_t at = part[t];
    for (int s = s0; s < s1; ++s) { pack[s] = at; at += totals[s]; }
}

// ---- the recorder's payload.  grid = (chunks, blocks, runs): block y of run z, every kept block with ITS OWN peak (one AudioThreadInput each)
CSDR_KERNEL_SQ __launch_bounds__(256) void squelch_pcm16(SquelchArgs a) {
    const SquelchRun &run = a.runs[blockIdx.z];
    if ((int)blockIdx.y >= run.n_blocks || run.audio == nullptr) return;
    const SquelchRec rc = a.recs[(size_t)run.slot * (size_t)a.max_blocks + blockIdx.y];
    if (rc.dst_off < 0) return;
    int16_t *dst = a.pcm + a.pack[run.slot] + rc.dst_off;
    if (rc.n < 0) {                                                                    // RECORD_SILENCE: zeros of the same length
        for (int i = blockIdx.x * 256 + threadIdx.x; i < -rc.n; i += 256 * gridDim.x) dst[i] = 0;
        return;
    }
    const float *src = run.audio + rc.src_off;
    const float scale = pcm16_scale(rc.peak);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < rc.n; i += 256 * gridDim.x) dst[i] = pcm16_sample(src[i], scale);
}

}  // namespace csdr
