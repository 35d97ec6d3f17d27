// csdr_specbank.hip -- implementation of include/csdr_hip.h (gfx950): csdr_specbank, N independent SpectrumVisualProcessors (full-span view) whose
// state and output stay in HBM.  The host plans every (slot, input) from the lengths alone -- which branch of the frame selection it takes
// (SpectrumVisualProcessor.cpp:387-421), where the peak-hold countdown stands (:247, :264-273) -- and uploads the plan as job records; ONE launch of
// specbank_process (kernels_specbank.hpp) does the arithmetic of all slots and all inputs of a call.  All work runs on a stream of the object's
// own, as the waterfall's does; the demodulator bank's resampled IQ is reached through bank_iq_acquire / _release (csdr_objects.hpp), ordered by events.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#define CSDR_TU_SPECBANK 1     // this unit is the home of its kernel (kernels_specbank.hpp)
#include "csdr_objects.hpp"
#include "kernels_specbank.hpp"

using namespace csdr;

static_assert(sizeof(csdr_specbank_item) == 24 && offsetof(csdr_specbank_item, iq) == 8 && offsetof(csdr_specbank_item, is_dev) == 16, "csdr_specbank_item layout");

namespace {
struct SbSlot {
    int last_size = 0;           // lastDataSize (setup :166)
    int peak_reset = 0;          // peakReset
    int frames = 0;              // frames of the last call
};
constexpr int kSbPeakResetCount = 30;        // PEAK_RESET_COUNT (SpectrumVisualProcessor.h:12)
constexpr int kSbStage = 2;                  // page-locked staging sets of the plan
}  // namespace

struct csdr_specbank {
    csdr_ctx *ctx = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;      // boundary stream -> st (device inputs of the caller), st -> boundary stream (csdr_specbank_device_points)
    bool ready = false;
    int F = 0, Fi = 0, max_slots = 0, max_frames = 0;
    float avg_rate = 0.65f, sf = 1.0f;                 // fft_average_rate (:36), scaleFactor
    float sf_last = 1.0f;                              // the scale factor the last call's frames were formed with (fft_ceiling = point_ceil / sf, :626)
    bool peak_hold = false;
    std::vector<SbSlot> slots;
    std::vector<int> touched;                          // slots that got frames in the last call
    DevBuf<float2> tw4096, last, stage;
    DevBuf<double> ma, maa, peak;
    DevBuf<SpecBankTrk> trk;
    DevBuf<float> points, hold;
    DevBuf<SpecBankFrame> meta;
    StageRing<kSbStage> plan;                          // SpecBankRun [runs] | SpecBankJob [jobs] of the call being run
    SpecBankTrk trk0{};                                // a fresh processor's trackers (the source of csdr_specbank_reset_slot's copy: stays)
    // scratch of a call's planning
    std::vector<SbSlot> work;
    std::vector<int> n_jobs_of, job_at, cursor, run_slots;     // per slot: jobs of the call, its first job, the next one to fill; the slots that have jobs
    std::vector<SpecBankJob> jobs_h;
    std::vector<csdr_specbank_item> bank_items;
    // a reader of `points` that stays on the device (specbank_points_acquire / _release: the waterfall bank's quantiser on its own stream).  Created
    // at the first acquire: a spectrum bank nobody reads this way never has them
    hipEvent_t ev_points_ready = nullptr, ev_points_read = nullptr;
    bool points_reader = false;                        // ev_points_read is recorded and not yet waited for
};

// whatever rewrites the points comes behind the reader that was handed them (one test, untaken while nobody reads this way)
static int sb_wait_reader(csdr_specbank *sb) {
    if (!sb->points_reader) return CSDR_OK;
    CSDR_HIP_TRY(hipStreamWaitEvent(sb->st, sb->ev_points_read, 0));
    sb->points_reader = false;
    return CSDR_OK;
}

extern "C" int csdr_specbank_create(csdr_ctx *ctx, csdr_specbank **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    std::unique_ptr<csdr_specbank> sb(new csdr_specbank());
    sb->ctx = ctx;
    CSDR_HIP_TRY(hipStreamCreateWithFlags(&sb->st, hipStreamNonBlocking));
    CSDR_HIP_TRY(hipEventCreateWithFlags(&sb->ev_in, hipEventDisableTiming));
    CSDR_HIP_TRY(hipEventCreateWithFlags(&sb->ev_out, hipEventDisableTiming));
    if (int rc = sb->plan.create()) return rc;
    sb->trk0.ceil_ma = sb->trk0.ceil_maa = 100.0;       // ctor :32
    sb->trk0.floor_ma = sb->trk0.floor_maa = 0.0;       // ctor :33
    sb->trk0.ceil_peak = sb->trk0.floor_peak = 0.0;     // (written by the reset of :264-273 before anything reads them)
    *out = sb.release();
    return CSDR_OK;
}

extern "C" void csdr_specbank_destroy(csdr_specbank *sb) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb) return;
    if (sb->st) { (void)hipStreamSynchronize(sb->st); (void)hipStreamDestroy(sb->st); }
    if (sb->ev_in) (void)hipEventDestroy(sb->ev_in);
    if (sb->ev_out) (void)hipEventDestroy(sb->ev_out);
    sb->plan.destroy();
    if (sb->ev_points_ready) (void)hipEventDestroy(sb->ev_points_ready);
    if (sb->ev_points_read) (void)hipEventDestroy(sb->ev_points_read);
    sb->tw4096.release(); sb->last.release(); sb->stage.release(); sb->ma.release(); sb->maa.release(); sb->peak.release(); sb->trk.release();
    sb->points.release(); sb->hold.release(); sb->meta.release();
    delete sb;
}

// a slot as SpectrumVisualProcessor's constructor and setup(fftSize_in) leave it (:9-38, :140-178), with setPeakHold(the object's setting) called once
static int sb_reset_slot(csdr_specbank *sb, int slot) {
    const size_t Fi = (size_t)sb->Fi, o = (size_t)slot * Fi;
    CSDR_HIP_TRY(hipMemsetAsync(sb->last.p + o, 0, Fi * sizeof(float2), sb->st));
    CSDR_HIP_TRY(hipMemsetAsync(sb->ma.p + o, 0, Fi * sizeof(double), sb->st));
    CSDR_HIP_TRY(hipMemsetAsync(sb->maa.p + o, 0, Fi * sizeof(double), sb->st));
    CSDR_HIP_TRY(hipMemsetAsync(sb->peak.p + o, 0, Fi * sizeof(double), sb->st));
    CSDR_HIP_TRY(hipMemcpyAsync(sb->trk.p + slot, &sb->trk0, sizeof(SpecBankTrk), hipMemcpyHostToDevice, sb->st));
    SbSlot &s = sb->slots[(size_t)slot];
    s.last_size = 0;
    s.peak_reset = 1;                                    // setPeakHold :115-125 on a processor whose peakHold was false
    s.frames = 0;
    return CSDR_OK;
}

extern "C" int csdr_specbank_setup(csdr_specbank *sb, int fft_size, int max_slots, int max_frames) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb) return fail(CSDR_EINVAL, "spectrum bank is null");
    if (fft_size < 8) return fail(CSDR_EINVAL, "fft_size %d: a power of two, 8 .. %d", fft_size, kFftMaxLds / 2);
    // sizes the reference takes and this object does not build (setFFTSize :180-190 takes any): the in-LDS transform holds 2 * fft_size <= 4096 points
    if ((fft_size & (fft_size - 1)) != 0 || fft_size > kFftMaxLds / 2) return fail(CSDR_EUNSUPPORTED, "fft_size %d: a power of two, 8 .. %d", fft_size, kFftMaxLds / 2);
    if (max_slots < 1 || max_slots > 4096) return fail(CSDR_EINVAL, "max_slots %d: 1 .. 4096", max_slots);
    if (max_frames < 1) return fail(CSDR_EINVAL, "max_frames %d", max_frames);
    if (int rc = sb_wait_reader(sb)) return rc;          // (the buffers may be replaced: the synchronise below then covers the reader too)
    CSDR_HIP_TRY(hipStreamSynchronize(sb->st));
    sb->ready = false;
    const size_t Fi = 2 * (size_t)fft_size, S = (size_t)max_slots;        // SPECTRUM_VZM (.h:11, :145)
    if (!sb->tw4096.p) {
        std::vector<float2> t(kTwTab);
        for (int i = 0; i < kTwTab; i++) { const double a = -2.0 * M_PI * i / kTwTab; t[(size_t)i] = make_float2((float)std::cos(a), (float)std::sin(a)); }
        if (int rc = sb->tw4096.reserve(kTwTab)) return rc;
        CSDR_HIP_TRY(hipMemcpy(sb->tw4096.p, t.data(), kTwTab * sizeof(float2), hipMemcpyHostToDevice));
    }
    if (int rc = sb->last.reserve(S * Fi)) return rc;
    if (int rc = sb->ma.reserve(S * Fi)) return rc;
    if (int rc = sb->maa.reserve(S * Fi)) return rc;
    if (int rc = sb->peak.reserve(S * Fi)) return rc;
    if (int rc = sb->trk.reserve(S)) return rc;
    if (int rc = sb->points.reserve(S * (size_t)max_frames * (size_t)fft_size)) return rc;
    if (int rc = sb->hold.reserve(S * (size_t)max_frames * (size_t)fft_size)) return rc;
    if (int rc = sb->meta.reserve(S * (size_t)max_frames)) return rc;
    sb->F = fft_size; sb->Fi = (int)Fi; sb->max_slots = max_slots; sb->max_frames = max_frames;
    sb->slots.assign(S, SbSlot());
    sb->touched.clear();
    // every slot a fresh processor: one fill per array, the trackers from a table
    CSDR_HIP_TRY(hipMemsetAsync(sb->last.p, 0, S * Fi * sizeof(float2), sb->st));
    CSDR_HIP_TRY(hipMemsetAsync(sb->ma.p, 0, S * Fi * sizeof(double), sb->st));
    CSDR_HIP_TRY(hipMemsetAsync(sb->maa.p, 0, S * Fi * sizeof(double), sb->st));
    CSDR_HIP_TRY(hipMemsetAsync(sb->peak.p, 0, S * Fi * sizeof(double), sb->st));
    std::vector<SpecBankTrk> t0(S, sb->trk0);
    CSDR_HIP_TRY(hipMemcpyAsync(sb->trk.p, t0.data(), S * sizeof(SpecBankTrk), hipMemcpyHostToDevice, sb->st));
    CSDR_HIP_TRY(hipStreamSynchronize(sb->st));          // (t0 is this call's)
    for (SbSlot &s : sb->slots) s.peak_reset = 1;
    CSDR_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(specbank_process), hipFuncAttributeMaxDynamicSharedMemorySize, (int)specbank_lds_bytes(kFftMaxLds)));
    sb->ready = true;
    return CSDR_OK;
}

extern "C" int csdr_specbank_set_average_rate(csdr_specbank *sb, float rate) {     // setFFTAverageRate
    if (!sb) return fail(CSDR_EINVAL, "spectrum bank is null");
    sb->avg_rate = rate;
    return CSDR_OK;
}
extern "C" int csdr_specbank_set_scale_factor(csdr_specbank *sb, float sf) {       // setScaleFactor
    if (!sb) return fail(CSDR_EINVAL, "spectrum bank is null");
    sb->sf = sf;
    return CSDR_OK;
}
extern "C" int csdr_specbank_set_peak_hold(csdr_specbank *sb, int enabled) {       // setPeakHold :115-125, on every slot
    if (!sb) return fail(CSDR_EINVAL, "spectrum bank is null");
    const bool again = sb->peak_hold && enabled;
    for (SbSlot &s : sb->slots) s.peak_reset = again ? kSbPeakResetCount : 1;
    if (!again) sb->peak_hold = enabled != 0;
    return CSDR_OK;
}
extern "C" int csdr_specbank_get_peak_hold(const csdr_specbank *sb) { return sb && sb->peak_hold ? 1 : 0; }

extern "C" int csdr_specbank_reset_slot(csdr_specbank *sb, int slot) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb || !sb->ready) return fail(CSDR_ESTATE, "spectrum bank not set up");
    if (slot < 0 || slot >= sb->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, sb->max_slots);
    if (int rc = sb_wait_reader(sb)) return rc;
    return sb_reset_slot(sb, slot);
}

// the plan and the launch of one call; `items` are checked.  any_dev: an input lies in device memory the caller produced on the boundary stream;
// bank: the inputs are that bank's resampled IQ -- acquired once the call can no longer be refused, released behind the kernel
static int sb_run(csdr_specbank *sb, const csdr_specbank_item *items, int n_items, bool any_dev, csdr_bank *bank = nullptr) {
    const int Fi = sb->Fi;
    // ---- plan on copies: a refused call leaves every slot as it was
    sb->work = sb->slots;
    sb->n_jobs_of.assign((size_t)sb->max_slots, 0);
    for (SbSlot &s : sb->work) s.frames = 0;
    size_t n_jobs = 0, host_samples = 0;
    for (int i = 0; i < n_items; ++i) {
        const csdr_specbank_item &it = items[i];
        if (it.n == 0) continue;                          // no input at all
        ++sb->n_jobs_of[(size_t)it.slot];
        ++n_jobs;
        if (!it.is_dev) host_samples += (size_t)std::min(it.n, Fi);
    }
    sb->run_slots.clear();
    sb->job_at.assign((size_t)sb->max_slots, 0);
    {
        int at = 0;
        for (int s = 0; s < sb->max_slots; ++s) if (sb->n_jobs_of[(size_t)s]) { sb->run_slots.push_back(s); sb->job_at[(size_t)s] = at; at += sb->n_jobs_of[(size_t)s]; }
    }
    sb->jobs_h.resize(n_jobs);
    sb->cursor = sb->job_at;
    for (int i = 0; i < n_items; ++i) {
        const csdr_specbank_item &it = items[i];
        if (it.n == 0) continue;
        SbSlot &s = sb->work[(size_t)it.slot];
        SpecBankJob jb{};
        jb.n = std::min(it.n, Fi);
        jb.do_peak = sb->peak_hold && s.peak_reset == 0 ? 1 : 0;              // :247
        if (s.peak_reset != 0 && --s.peak_reset == 0) jb.peak_reset_now = 1;  // :264-273
        if (it.n >= Fi) { jb.action = kSbFull; jb.arg = 0; }                  // :401-404 (lastDataSize is not touched)
        else if (s.last_size + it.n < Fi) {                                   // priming :407-413
            jb.action = kSbPrime;
            jb.arg = std::max(Fi - s.last_size, it.n);
            s.last_size += jb.arg;
        } else {                                                              // :415-419
            if (s.last_size > Fi) return fail(CSDR_ESTATE, "slot %d: lastDataSize %d beyond %d", it.slot, s.last_size, Fi);      // (cannot happen: priming stops at Fi)
            jb.action = kSbSlide;
            jb.arg = s.last_size - (Fi - it.n);
        }
        jb.frame = jb.action == kSbPrime ? -1 : s.frames++;
        jb.src = it.is_dev ? reinterpret_cast<const float2 *>(it.iq) : nullptr;       // (a host input: its place in the staging buffer, below)
        sb->jobs_h[(size_t)sb->cursor[(size_t)it.slot]++] = jb;
    }
    for (int s : sb->run_slots)
        if (sb->work[(size_t)s].frames > sb->max_frames)
            return fail(CSDR_ERANGE, "slot %d: %d frames in one call exceed max_frames %d", s, sb->work[(size_t)s].frames, sb->max_frames);
    // ---- commit the host state; from here on the call is enqueued
    for (int s : sb->touched) sb->slots[(size_t)s].frames = 0;
    sb->touched = sb->run_slots;
    for (int s : sb->run_slots) sb->slots[(size_t)s] = sb->work[(size_t)s];
    sb->sf_last = sb->sf;
    if (n_jobs == 0) return CSDR_OK;
    if (int rc = sb_wait_reader(sb)) return rc;
    if (bank) if (int rc = bank_iq_acquire(bank, sb->st)) return rc;
    if (any_dev) {
        CSDR_HIP_TRY(hipEventRecord(sb->ev_in, sb->ctx->stream));
        CSDR_HIP_TRY(hipStreamWaitEvent(sb->st, sb->ev_in, 0));
    }
    if (host_samples) {
        if (host_samples > sb->stage.cap) CSDR_HIP_TRY(hipStreamSynchronize(sb->st));        // (a kernel may still read the buffer being replaced)
        if (int rc = sb->stage.reserve(host_samples)) return rc;
    }
    if (host_samples) {                                   // host inputs, staged in item order
        size_t at = 0;
        sb->cursor = sb->job_at;
        for (int i = 0; i < n_items; ++i) {
            const csdr_specbank_item &it = items[i];
            if (it.n == 0) continue;
            SpecBankJob &jb = sb->jobs_h[(size_t)sb->cursor[(size_t)it.slot]++];
            if (it.is_dev) continue;
            float2 *dst = sb->stage.p + at;
            CSDR_HIP_TRY(hipMemcpyAsync(dst, it.iq, (size_t)jb.n * sizeof(float2), hipMemcpyHostToDevice, sb->st));
            jb.src = dst;
            at += (size_t)jb.n;
        }
    }
    const size_t n_runs = sb->run_slots.size();
    const size_t bytes = n_runs * sizeof(SpecBankRun) + n_jobs * sizeof(SpecBankJob);
    if (int rc = sb->plan.begin(sb->st, bytes)) return rc;           // the one host wait of a call
    SpecBankRun *runs_h = reinterpret_cast<SpecBankRun *>(sb->plan.host());
    for (size_t r = 0; r < n_runs; ++r) {
        const int s = sb->run_slots[r];
        runs_h[r] = SpecBankRun{s, sb->job_at[(size_t)s], sb->n_jobs_of[(size_t)s], 0};
    }
    memcpy(sb->plan.host() + n_runs * sizeof(SpecBankRun), sb->jobs_h.data(), n_jobs * sizeof(SpecBankJob));
    if (int rc = sb->plan.uploaded(sb->st, bytes)) return rc;
    SpecBankArgs a{};
    a.runs = reinterpret_cast<const SpecBankRun *>(sb->plan.device());
    a.jobs = reinterpret_cast<const SpecBankJob *>(sb->plan.device() + n_runs * sizeof(SpecBankRun));
    a.tw4096 = sb->tw4096.p;
    a.last = sb->last.p; a.ma = sb->ma.p; a.maa = sb->maa.p; a.peak = sb->peak.p; a.trk = sb->trk.p;
    a.points = sb->points.p; a.hold = sb->hold.p; a.meta = sb->meta.p;
    a.Fi = Fi; a.max_frames = sb->max_frames; a.rate = (double)sb->avg_rate; a.sf = sb->sf;
    {
        ProfScope ps__(sb->ctx, KID_SPECBANK, sb->st);
        hipLaunchKernelGGL(specbank_process, dim3((unsigned)n_runs), dim3(kFftThreads), specbank_lds_bytes(Fi), sb->st, a);
    }
    CSDR_HIP_TRY(hipGetLastError());
    return bank ? bank_iq_release(bank, sb->st) : CSDR_OK;
}

extern "C" int csdr_specbank_process(csdr_specbank *sb, const csdr_specbank_item *items, int n_items) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb || !sb->ready) return fail(CSDR_ESTATE, "spectrum bank not set up");
    if (n_items < 0 || (n_items > 0 && !items)) return fail(CSDR_EINVAL, "bad items");
    bool any_dev = false;
    for (int i = 0; i < n_items; ++i) {
        const csdr_specbank_item &it = items[i];
        if (it.slot < 0 || it.slot >= sb->max_slots) return fail(CSDR_EINVAL, "item %d: slot %d of %d", i, it.slot, sb->max_slots);
        if (it.n < 0 || (it.n > 0 && !it.iq)) return fail(CSDR_EINVAL, "item %d: %d samples at %p", i, it.n, (const void *)it.iq);
        if (it.n > 0 && it.is_dev) {
            if ((uintptr_t)it.iq & 7) return fail(CSDR_EINVAL, "item %d: device samples must be 8-byte aligned", i);
            any_dev = true;
        }
    }
    return sb_run(sb, items, n_items, any_dev);
}

extern "C" int csdr_specbank_process_bank(csdr_specbank *sb, csdr_bank *bank) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb || !sb->ready) return fail(CSDR_ESTATE, "spectrum bank not set up");
    if (!bank) return fail(CSDR_EINVAL, "bank is null");
    if (bank->ctx != sb->ctx) return fail(CSDR_EINVAL, "the bank belongs to another context");
    if (bank->last_nb == 0) return fail(CSDR_ESTATE, "no csdr_bank_execute yet");
    // one item per block of the last execute for every active slot the object has room for; a block the front-end skipped has no samples: no input
    sb->bank_items.clear();
    const int ns = std::min(sb->max_slots, bank->max_demods);
    for (int si = 0; si < ns; ++si) {
        const SlotHost &s = bank->slots[(size_t)si];
        if (!s.configured || !s.active || s.results.empty() || s.last_J == 0) continue;
        const float2 *cur = bank_slot_iq(s);
        int64_t j0 = 0;
        for (const csdr_block_result &r : s.results) {
            if (!r.skipped && r.n_iq > 0) sb->bank_items.push_back(csdr_specbank_item{si, r.n_iq, reinterpret_cast<const float *>(cur + j0), 1});
            j0 += r.n_iq;
        }
    }
    if (sb->bank_items.empty()) return sb_run(sb, nullptr, 0, false);
    return sb_run(sb, sb->bank_items.data(), (int)sb->bank_items.size(), false, bank);
}

extern "C" int csdr_specbank_frames(const csdr_specbank *sb, int slot) {
    return sb && sb->ready && slot >= 0 && slot < sb->max_slots ? sb->slots[(size_t)slot].frames : 0;
}

static int sb_check_frame(const csdr_specbank *sb, int slot, int frame) {
    if (!sb || !sb->ready) return fail(CSDR_ESTATE, "spectrum bank not set up");
    if (slot < 0 || slot >= sb->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, sb->max_slots);
    if (frame < 0 || frame >= sb->slots[(size_t)slot].frames) return fail(CSDR_EINVAL, "frame %d of %d", frame, sb->slots[(size_t)slot].frames);
    return CSDR_OK;
}

// SpectrumVisualData of a frame: the device keeps only the y of every point; the x of point i is (float)i / (float)fftSize (:563)
static int sb_fetch(csdr_specbank *sb, const float *src, size_t fo, float *host, SpecBankFrame *m) {
    const int F = sb->F;
    CSDR_HIP_TRY(hipMemcpyAsync(host + F, src + fo * (size_t)F, (size_t)F * sizeof(float), hipMemcpyDeviceToHost, sb->st));
    CSDR_HIP_TRY(hipMemcpyAsync(m, sb->meta.p + fo, sizeof(SpecBankFrame), hipMemcpyDeviceToHost, sb->st));
    CSDR_HIP_TRY(hipStreamSynchronize(sb->st));
    for (int i = 0; i < F; ++i) { const float y = host[F + i]; host[2 * i] = (float)i / (float)F; host[2 * i + 1] = y; }
    return CSDR_OK;
}

extern "C" int csdr_specbank_fetch(csdr_specbank *sb, int slot, int frame, float *points_host, int cap_floats, double *fft_ceiling, double *fft_floor) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (int rc = sb_check_frame(sb, slot, frame)) return rc;
    if (!points_host) return fail(CSDR_EINVAL, "null argument");
    if (cap_floats < 2 * sb->F) return fail(CSDR_ERANGE, "need room for %d floats", 2 * sb->F);
    SpecBankFrame m{};
    const size_t fo = (size_t)slot * (size_t)sb->max_frames + (size_t)frame;
    if (int rc = sb_fetch(sb, sb->points.p, fo, points_host, &m)) return rc;
    if (fft_ceiling) *fft_ceiling = m.point_ceil / sb->sf_last;          // :626
    if (fft_floor) *fft_floor = m.point_floor;                           // :627
    return CSDR_OK;
}

extern "C" int csdr_specbank_fetch_hold(csdr_specbank *sb, int slot, int frame, float *hold_host, int cap_floats, int *n_floats) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (n_floats) *n_floats = 0;
    if (int rc = sb_check_frame(sb, slot, frame)) return rc;
    if (!hold_host || !n_floats) return fail(CSDR_EINVAL, "null argument");
    if (cap_floats < 2 * sb->F) return fail(CSDR_ERANGE, "need room for %d floats", 2 * sb->F);
    SpecBankFrame m{};
    const size_t fo = (size_t)slot * (size_t)sb->max_frames + (size_t)frame;
    if (int rc = sb_fetch(sb, sb->hold.p, fo, hold_host, &m)) return rc;
    *n_floats = m.hold ? 2 * sb->F : 0;
    return CSDR_OK;
}

extern "C" int csdr_specbank_device_points(csdr_specbank *sb, int slot, const float **dev, int *frames) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb || !sb->ready) return fail(CSDR_ESTATE, "spectrum bank not set up");
    if (!dev || slot < 0 || slot >= sb->max_slots) return fail(CSDR_EINVAL, "bad argument");
    CSDR_HIP_TRY(hipEventRecord(sb->ev_out, sb->st));     // whatever the caller enqueues on the boundary stream next reads the finished points
    CSDR_HIP_TRY(hipStreamWaitEvent(sb->ctx->stream, sb->ev_out, 0));
    *dev = sb->points.p + (size_t)slot * (size_t)sb->max_frames * (size_t)sb->F;
    if (frames) *frames = sb->slots[(size_t)slot].frames;
    return CSDR_OK;
}

// ---- the points for a reader that stays on the device (csdr_objects.hpp) ----
int specbank_points_acquire(csdr_specbank *sb, hipStream_t reader, SpecBankPointsRef *out) {
    if (!sb || !sb->ready || !out) return fail(CSDR_ESTATE, "spectrum bank not set up");
    if (!sb->ev_points_ready) {
        CSDR_HIP_TRY(hipEventCreateWithFlags(&sb->ev_points_ready, hipEventDisableTiming));
        CSDR_HIP_TRY(hipEventCreateWithFlags(&sb->ev_points_read, hipEventDisableTiming));
    }
    CSDR_HIP_TRY(hipEventRecord(sb->ev_points_ready, sb->st));
    CSDR_HIP_TRY(hipStreamWaitEvent(reader, sb->ev_points_ready, 0));
    out->ctx = sb->ctx; out->points = sb->points.p; out->F = sb->F; out->max_slots = sb->max_slots; out->max_frames = sb->max_frames;
    return CSDR_OK;
}
int specbank_points_release(csdr_specbank *sb, hipStream_t reader) {
    CSDR_HIP_TRY(hipEventRecord(sb->ev_points_read, reader));
    sb->points_reader = true;
    return CSDR_OK;
}
