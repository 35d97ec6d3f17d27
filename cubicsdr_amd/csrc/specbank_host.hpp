// specbank_host.hpp -- the host side of a bank of SpectrumVisualProcessors (src/process/SpectrumVisualProcessor.cpp) that csdr_specbank.hip (full-span
// view) and csdr_viewbank.hip (zoomed view) both are, stated once: the per-slot frame store in HBM, the peak-hold countdown, the frame rule, the slot
// order of a call with its staging and upload, and the fetches.  Internal to those two units; the device-side counterpart is the sb_* functions of
// kernels_specbank.hpp.  What differs stays in the units: where the inputs come from (the demodulator bank's IQ / a channelizer's rows), the view
// plan and the resamplers of the view bank, the device-side reader of the spectrum bank's points.
#pragma once
#include <algorithm>
#include <vector>

#include "csdr_objects.hpp"
#include "kernels_specbank.hpp"

namespace csdr {

constexpr int kSbPeakResetCount = 30;        // PEAK_RESET_COUNT (SpectrumVisualProcessor.h:12)
constexpr int kSbStage = 2;                  // page-locked staging sets of the plan

struct SbSlot {                              // the processor's integers that both views keep
    int last_size = 0;                       // lastDataSize (setup :166)
    int peak_reset = 0;                      // peakReset
    int frames = 0;                          // frames of the last call
};

// what setup takes of (fft_size, max_slots, max_frames)
inline int sb_check_setup(int fft_size, int max_slots, int max_frames) {
    if (fft_size < 8) return fail(CSDR_EINVAL, "fft_size %d: a power of two, 8 .. %d", fft_size, kFftMaxLds / 2);
    // sizes the reference takes and these objects do not build (setFFTSize :180-190 takes any): the in-LDS transform holds 2 * fft_size <= 4096 points
    if ((fft_size & (fft_size - 1)) != 0 || fft_size > kFftMaxLds / 2) return fail(CSDR_EUNSUPPORTED, "fft_size %d: a power of two, 8 .. %d", fft_size, kFftMaxLds / 2);
    if (max_slots < 1 || max_slots > 4096) return fail(CSDR_EINVAL, "max_slots %d: 1 .. 4096", max_slots);
    if (max_frames < 1) return fail(CSDR_EINVAL, "max_frames %d", max_frames);
    return CSDR_OK;
}

// the items of a process call, before anything is planned; any_dev: an input lies in device memory
template <typename Item>
int sb_check_items(const Item *items, int n_items, int max_slots, bool *any_dev) {
    if (n_items < 0 || (n_items > 0 && !items)) return fail(CSDR_EINVAL, "bad items");
    *any_dev = false;
    for (int i = 0; i < n_items; ++i) {
        const Item &it = items[i];
        if (it.slot < 0 || it.slot >= max_slots) return fail(CSDR_EINVAL, "item %d: slot %d of %d", i, it.slot, max_slots);
        if (it.n < 0 || (it.n > 0 && !it.iq)) return fail(CSDR_EINVAL, "item %d: %d samples at %p", i, it.n, (const void *)it.iq);
        if (it.n > 0 && it.is_dev) {
            if ((uintptr_t)it.iq & 7) return fail(CSDR_EINVAL, "item %d: device samples must be 8-byte aligned", i);
            *any_dev = true;
        }
    }
    return CSDR_OK;
}

// The object both banks derive from.  Slot: SbSlot or a struct derived from it; Job: SpecBankJob or ViewBankJob (the fields the two share are
// named alike).  All work runs on `st`, the side stream (ev_in: a producer's stream -> st for device inputs; ev_out: device_points); the slot order
// of a call is SlotOrder's (stream_order.hpp).
template <typename Slot, typename Job>
struct SbBank : SideStream, SlotOrder {
    bool ready = false;
    int F = 0, Fi = 0, max_slots = 0, max_frames = 0;
    float avg_rate = 0.65f, sf = 1.0f;                 // fft_average_rate (:36), scaleFactor
    float sf_last = 1.0f;                              // the scale factor the last call's frames were formed with (fft_ceiling = point_ceil / sf, :626)
    bool peak_hold = false;
    std::vector<Slot> slots;
    // ---- the per-slot frame store
    DevBuf<float2> tw4096, last, stage;                // (stage: the host inputs of a call)
    DevBuf<double> ma, maa, peak;
    DevBuf<SpecBankTrk> trk;
    DevBuf<float> points, hold;
    DevBuf<SpecBankFrame> meta;
    SpecBankTrk trk0{};                                // a fresh processor's trackers (the source of reset_frames' copy: stays)
    // ---- a call's plan
    StageRing<kSbStage> plan;                          // SpecBankRun [runs] | Job [jobs] of the call being run
    std::vector<Slot> work;                            // copies the call is planned on
    std::vector<Job> jobs_h;

    int create_base(csdr_ctx *c) {
        if (int rc = SideStream::create(c)) return rc;
        if (int rc = plan.create()) return rc;
        trk0.ceil_ma = trk0.ceil_maa = 100.0;           // ctor :32
        trk0.floor_ma = trk0.floor_maa = 0.0;           // ctor :33
        trk0.ceil_peak = trk0.floor_peak = 0.0;         // (written by the reset of :264-273 before anything reads them)
        return CSDR_OK;
    }
    void destroy_base() {
        SideStream::destroy();
        plan.destroy();
        tw4096.release(); last.release(); stage.release(); ma.release(); maa.release(); peak.release(); trk.release();
        points.release(); hold.release(); meta.release();
    }

    // room for max_slots_in processors of fft_size with max_frames_in frames per call
    int reserve_frames(int fft_size, int max_slots_in, int max_frames_in) {
        const size_t Fi_ = 2 * (size_t)fft_size, S = (size_t)max_slots_in;    // SPECTRUM_VZM (.h:11, :145)
        if (int rc = upload_twiddles(tw4096, kTwTab)) return rc;
        if (int rc = last.reserve(S * Fi_)) return rc;
        if (int rc = ma.reserve(S * Fi_)) return rc;
        if (int rc = maa.reserve(S * Fi_)) return rc;
        if (int rc = peak.reserve(S * Fi_)) return rc;
        if (int rc = trk.reserve(S)) return rc;
        if (int rc = points.reserve(S * (size_t)max_frames_in * (size_t)fft_size)) return rc;
        if (int rc = hold.reserve(S * (size_t)max_frames_in * (size_t)fft_size)) return rc;
        if (int rc = meta.reserve(S * (size_t)max_frames_in)) return rc;
        F = fft_size; Fi = (int)Fi_; max_slots = max_slots_in; max_frames = max_frames_in;
        return CSDR_OK;
    }
    // every slot a fresh processor on which setPeakHold was called once: one fill per array, the trackers from a table.  Ends in a synchronise
    int fresh_slots() {
        const size_t S = (size_t)max_slots, n = S * (size_t)Fi;
        slots.assign(S, Slot());
        touched.clear();
        CSDR_HIP_TRY(hipMemsetAsync(last.p, 0, n * sizeof(float2), st));
        CSDR_HIP_TRY(hipMemsetAsync(ma.p, 0, n * sizeof(double), st));
        CSDR_HIP_TRY(hipMemsetAsync(maa.p, 0, n * sizeof(double), st));
        CSDR_HIP_TRY(hipMemsetAsync(peak.p, 0, n * sizeof(double), st));
        std::vector<SpecBankTrk> t0(S, trk0);
        CSDR_HIP_TRY(hipMemcpyAsync(trk.p, t0.data(), S * sizeof(SpecBankTrk), hipMemcpyHostToDevice, st));
        CSDR_HIP_TRY(hipStreamSynchronize(st));          // (t0 is this call's)
        for (Slot &s : slots) s.peak_reset = 1;
        return CSDR_OK;
    }
    // a slot's arrays as SpectrumVisualProcessor's constructor and setup(fftSize_in) leave them (:9-38, :140-178); the slot's integers: the caller
    int reset_frames(int slot) {
        const size_t n = (size_t)Fi, o = (size_t)slot * n;
        CSDR_HIP_TRY(hipMemsetAsync(last.p + o, 0, n * sizeof(float2), st));
        CSDR_HIP_TRY(hipMemsetAsync(ma.p + o, 0, n * sizeof(double), st));
        CSDR_HIP_TRY(hipMemsetAsync(maa.p + o, 0, n * sizeof(double), st));
        CSDR_HIP_TRY(hipMemsetAsync(peak.p + o, 0, n * sizeof(double), st));
        CSDR_HIP_TRY(hipMemcpyAsync(trk.p + slot, &trk0, sizeof(SpecBankTrk), hipMemcpyHostToDevice, st));
        return CSDR_OK;
    }

    // setPeakHold :115-125, on every slot
    void set_peak_hold(int enabled) {
        const bool again = peak_hold && enabled;
        for (Slot &s : slots) s.peak_reset = again ? kSbPeakResetCount : 1;
        if (!again) peak_hold = enabled != 0;
    }

    // behind the count (SlotOrder): where every slot's jobs lie, and the copies of the slots that run (a refused call leaves every slot as it was)
    void order_jobs() {
        jobs_h.resize(order());
        work.resize((size_t)max_slots);
        for (int s : run_slots) { work[(size_t)s] = slots[(size_t)s]; work[(size_t)s].frames = 0; }
    }

    // the head of process() for one input: doPeak (:247) and the countdown (:264-273)
    void job_head(Job &jb, Slot &s) const {
        jb.do_peak = peak_hold && s.peak_reset == 0 ? 1 : 0;
        if (s.peak_reset != 0 && --s.peak_reset == 0) jb.peak_reset_now = 1;
    }
    // the frame rule (:399-421) for n fresh samples: which branch, its argument, the frame the input makes (none while priming)
    int frame_rule(Job &jb, Slot &s, int slot, int n) const {
        if (n >= Fi) { jb.action = kSbFull; jb.arg = 0; }                     // :401-404 (lastDataSize is not touched)
        else if (s.last_size + n < Fi) {                                      // priming :407-413
            jb.action = kSbPrime;
            jb.arg = std::max(Fi - s.last_size, n);
            s.last_size += jb.arg;
        } else {                                                              // :415-419
            if (s.last_size > Fi) return fail(CSDR_ESTATE, "slot %d: lastDataSize %d beyond %d", slot, s.last_size, Fi);      // (cannot happen: priming stops at Fi)
            jb.action = kSbSlide;
            jb.arg = s.last_size - (Fi - n);
        }
        jb.frame = jb.action == kSbPrime ? -1 : s.frames++;
        return CSDR_OK;
    }
    int check_frames() const {
        for (int s : run_slots)
            if (work[(size_t)s].frames > max_frames)
                return fail(CSDR_ERANGE, "slot %d: %d frames in one call exceed max_frames %d", s, work[(size_t)s].frames, max_frames);
        return CSDR_OK;
    }
    // the planned call becomes the slots' state; from here on the call is enqueued
    void commit() {
        SlotOrder::commit([&](int s) { slots[(size_t)s].frames = 0; }, [&](int s) { slots[(size_t)s] = work[(size_t)s]; });
        sf_last = sf;
    }

    // host inputs, staged in item order: the jb.n samples each job consumes (a job that consumes none has nothing to stage)
    template <typename Item>
    int stage_inputs(const Item *items, int n_items, size_t host_samples) {
        if (!host_samples) return CSDR_OK;
        if (host_samples > stage.cap) CSDR_HIP_TRY(hipStreamSynchronize(st));        // (a kernel may still read the buffer being replaced)
        if (int rc = stage.reserve(host_samples)) return rc;
        size_t at = 0;
        rewind();
        for (int i = 0; i < n_items; ++i) {
            const Item &it = items[i];
            if (it.n == 0) continue;
            Job &jb = jobs_h[next_job(it.slot)];
            if (it.is_dev || jb.n == 0) continue;
            float2 *dst = stage.p + at;
            CSDR_HIP_TRY(hipMemcpyAsync(dst, it.iq, (size_t)jb.n * sizeof(float2), hipMemcpyHostToDevice, st));
            jb.src = dst;
            at += (size_t)jb.n;
        }
        return CSDR_OK;
    }
    // runs | jobs through the staging ring; begin() holds the one host wait of a call
    int upload_plan(const SpecBankRun **runs_d, const Job **jobs_d) {
        const size_t n_jobs = jobs_h.size(), bytes = run_bytes() + n_jobs * sizeof(Job);
        if (int rc = plan.begin(st, bytes)) return rc;
        fill_runs(plan.host());
        memcpy(plan.host() + run_bytes(), jobs_h.data(), n_jobs * sizeof(Job));
        if (int rc = plan.uploaded(st, bytes)) return rc;
        *runs_d = reinterpret_cast<const SpecBankRun *>(plan.device());
        *jobs_d = reinterpret_cast<const Job *>(plan.device() + run_bytes());
        return CSDR_OK;
    }
    // the frame store's part of the kernel arguments (SpecBankArgs and ViewBankArgs name these fields alike)
    template <typename Args>
    void fill_args(Args &a) const {
        a.tw4096 = tw4096.p;
        a.last = last.p; a.ma = ma.p; a.maa = maa.p; a.peak = peak.p; a.trk = trk.p;
        a.points = points.p; a.hold = hold.p; a.meta = meta.p;
        a.Fi = Fi; a.max_frames = max_frames; a.rate = (double)avg_rate; a.sf = sf;
    }
};

// ---- the entry points both banks have, on a pointer to either object (Bank::kName: how its messages call it) ----
template <typename Bank>
int sb_check_ready(const Bank *b) { return b && b->ready ? CSDR_OK : fail(CSDR_ESTATE, "%s not set up", Bank::kName); }
template <typename Bank>
int sb_check_slot(const Bank *b, int slot) {
    if (int rc = sb_check_ready(b)) return rc;
    if (slot < 0 || slot >= b->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, b->max_slots);
    return CSDR_OK;
}
template <typename Bank>
int sb_check_frame(const Bank *b, int slot, int frame) {
    if (int rc = sb_check_slot(b, slot)) return rc;
    if (frame < 0 || frame >= b->slots[(size_t)slot].frames) return fail(CSDR_EINVAL, "frame %d of %d", frame, b->slots[(size_t)slot].frames);
    return CSDR_OK;
}
template <typename Bank>
int sb_frames(const Bank *b, int slot) { return b && b->ready && slot >= 0 && slot < b->max_slots ? b->slots[(size_t)slot].frames : 0; }

// SpectrumVisualData of a frame: the device keeps only the y of every point; the x of point i is (float)i / (float)fftSize (:563)
template <typename Bank>
int sb_fetch_frame(Bank *b, const float *src, int slot, int frame, float *host, int cap_floats, SpecBankFrame *m) {
    const int F = b->F;
    if (cap_floats < 2 * F) return fail(CSDR_ERANGE, "need room for %d floats", 2 * F);
    const size_t fo = (size_t)slot * (size_t)b->max_frames + (size_t)frame;
    CSDR_HIP_TRY(hipMemcpyAsync(host + F, src + fo * (size_t)F, (size_t)F * sizeof(float), hipMemcpyDeviceToHost, b->st));
    CSDR_HIP_TRY(hipMemcpyAsync(m, b->meta.p + fo, sizeof(SpecBankFrame), hipMemcpyDeviceToHost, b->st));
    CSDR_HIP_TRY(hipStreamSynchronize(b->st));
    for (int i = 0; i < F; ++i) { const float y = host[F + i]; host[2 * i] = (float)i / (float)F; host[2 * i + 1] = y; }
    return CSDR_OK;
}
template <typename Bank>
int sb_fetch(Bank *b, int slot, int frame, float *points_host, int cap_floats, double *fft_ceiling, double *fft_floor) {
    if (int rc = sb_check_frame(b, slot, frame)) return rc;
    if (!points_host) return fail(CSDR_EINVAL, "null argument");
    SpecBankFrame m{};
    if (int rc = sb_fetch_frame(b, b->points.p, slot, frame, points_host, cap_floats, &m)) return rc;
    if (fft_ceiling) *fft_ceiling = m.point_ceil / b->sf_last;           // :626
    if (fft_floor) *fft_floor = m.point_floor;                           // :627
    return CSDR_OK;
}
template <typename Bank>
int sb_fetch_hold(Bank *b, int slot, int frame, float *hold_host, int cap_floats, int *n_floats) {
    if (n_floats) *n_floats = 0;
    if (int rc = sb_check_frame(b, slot, frame)) return rc;
    if (!hold_host || !n_floats) return fail(CSDR_EINVAL, "null argument");
    SpecBankFrame m{};
    if (int rc = sb_fetch_frame(b, b->hold.p, slot, frame, hold_host, cap_floats, &m)) return rc;
    *n_floats = m.hold ? 2 * b->F : 0;
    return CSDR_OK;
}
template <typename Bank>
int sb_device_points(Bank *b, int slot, const float **dev, int *frames) {
    if (int rc = sb_check_ready(b)) return rc;
    if (!dev || slot < 0 || slot >= b->max_slots) return fail(CSDR_EINVAL, "bad argument");
    if (int rc = b->hand_over()) return rc;               // whatever the caller enqueues on the boundary stream next reads the finished points
    *dev = b->points.p + (size_t)slot * (size_t)b->max_frames * (size_t)b->F;
    if (frames) *frames = b->slots[(size_t)slot].frames;
    return CSDR_OK;
}

}  // namespace csdr
