// csdr_specbank.hip -- implementation of include/csdr_hip.h (gfx950): csdr_specbank, N independent SpectrumVisualProcessors (full-span view) whose
// state and output stay in HBM.  The host plans every (slot, input) from the lengths alone -- which branch of the frame selection it takes
// (SpectrumVisualProcessor.cpp:387-421), where the peak-hold countdown stands (:247, :264-273) -- and uploads the plan as job records; ONE launch of
// specbank_process (kernels_specbank.hpp) does the arithmetic of all slots and all inputs of a call.  All work runs on a stream of the object's
// own, as the waterfall's does; the demodulator bank's resampled IQ is reached through bank_iq_acquire / _release (csdr_objects.hpp), ordered by events.
// The frame store, the countdown, the frame rule, the slot order of a call and the fetches are specbank_host.hpp's, shared with csdr_viewbank.hip.
#include <algorithm>
#include <memory>
#include <vector>

#define CSDR_TU_SPECBANK 1     // this unit is the home of its kernel (kernels_specbank.hpp)
#include "specbank_host.hpp"

using namespace csdr;

static_assert(sizeof(csdr_specbank_item) == 24 && offsetof(csdr_specbank_item, iq) == 8 && offsetof(csdr_specbank_item, is_dev) == 16, "csdr_specbank_item layout");

struct csdr_specbank : SbBank<SbSlot, SpecBankJob> {
    static constexpr const char *kName = "spectrum bank";
    std::vector<csdr_specbank_item> bank_items;
    ReadGate points_gate;                              // readers of `points` that stay on the device (specbank_points_acquire / _release: the waterfall bank's quantiser on its own stream)
};

// whatever rewrites the points comes behind the readers that were handed them
static int sb_wait_reader(csdr_specbank *sb) { return sb->points_gate.wait(sb->st); }

extern "C" int csdr_specbank_create(csdr_ctx *ctx, csdr_specbank **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    std::unique_ptr<csdr_specbank, void (*)(csdr_specbank *)> sb(new csdr_specbank(), csdr_specbank_destroy);
    if (int rc = sb->create_base(ctx)) return rc;
    *out = sb.release();
    return CSDR_OK;
}

extern "C" void csdr_specbank_destroy(csdr_specbank *sb) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb) return;
    sb->points_gate.destroy();                           // (host-waits for a reader on a stream that is not the object's)
    sb->destroy_base();
    delete sb;
}

extern "C" int csdr_specbank_setup(csdr_specbank *sb, int fft_size, int max_slots, int max_frames) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb) return fail(CSDR_EINVAL, "spectrum bank is null");
    if (int rc = sb_check_setup(fft_size, max_slots, max_frames)) return rc;
    if (int rc = sb_wait_reader(sb)) return rc;          // (the buffers may be replaced: the synchronise below then covers the reader too)
    CSDR_HIP_TRY(hipStreamSynchronize(sb->st));
    sb->ready = false;
    if (int rc = sb->reserve_frames(fft_size, max_slots, max_frames)) return rc;
    if (int rc = sb->fresh_slots()) return rc;
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
extern "C" int csdr_specbank_set_peak_hold(csdr_specbank *sb, int enabled) {
    if (!sb) return fail(CSDR_EINVAL, "spectrum bank is null");
    sb->set_peak_hold(enabled);
    return CSDR_OK;
}
extern "C" int csdr_specbank_get_peak_hold(const csdr_specbank *sb) { return sb && sb->peak_hold ? 1 : 0; }

// a slot as a fresh processor, with setPeakHold(the object's setting) called once
extern "C" int csdr_specbank_reset_slot(csdr_specbank *sb, int slot) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (int rc = sb_check_slot(sb, slot)) return rc;
    if (int rc = sb_wait_reader(sb)) return rc;
    if (int rc = sb->reset_frames(slot)) return rc;
    SbSlot fresh;
    fresh.peak_reset = 1;                                // setPeakHold :115-125 on a processor whose peakHold was false
    sb->slots[(size_t)slot] = fresh;
    return CSDR_OK;
}

// the plan and the launch of one call; `items` are checked.  any_dev: an input lies in device memory the caller produced on the boundary stream;
// bank: the inputs are that bank's resampled IQ -- acquired once the call can no longer be refused, released behind the kernel
static int sb_run(csdr_specbank *sb, const csdr_specbank_item *items, int n_items, bool any_dev, csdr_bank *bank = nullptr) {
    const int Fi = sb->Fi;
    // ---- plan on copies: a refused call leaves every slot as it was
    sb->count_begin(sb->max_slots);
    size_t n_jobs = 0, host_samples = 0;
    for (int i = 0; i < n_items; ++i) {
        const csdr_specbank_item &it = items[i];
        if (it.n == 0) continue;                          // no input at all
        sb->count_job(it.slot);
        ++n_jobs;
        if (!it.is_dev) host_samples += (size_t)std::min(it.n, Fi);
    }
    sb->order_jobs();
    for (int i = 0; i < n_items; ++i) {
        const csdr_specbank_item &it = items[i];
        if (it.n == 0) continue;
        SbSlot &s = sb->work[(size_t)it.slot];
        SpecBankJob jb{};
        jb.n = std::min(it.n, Fi);
        sb->job_head(jb, s);
        if (int rc = sb->frame_rule(jb, s, it.slot, it.n)) return rc;
        jb.src = it.is_dev ? reinterpret_cast<const float2 *>(it.iq) : nullptr;       // (a host input: its place in the staging buffer, below)
        sb->jobs_h[sb->next_job(it.slot)] = jb;
    }
    if (int rc = sb->check_frames()) return rc;
    sb->commit();
    if (n_jobs == 0) return CSDR_OK;
    if (int rc = sb_wait_reader(sb)) return rc;
    if (bank) if (int rc = bank_iq_acquire(bank, sb->st)) return rc;
    if (any_dev) if (int rc = sb->after_boundary()) return rc;
    if (int rc = sb->stage_inputs(items, n_items, host_samples)) return rc;
    SpecBankArgs a{};
    if (int rc = sb->upload_plan(&a.runs, &a.jobs)) return rc;
    sb->fill_args(a);
    {
        ProfScope ps__(sb->ctx, KID_SPECBANK, sb->st);
        hipLaunchKernelGGL(specbank_process, dim3((unsigned)sb->run_slots.size()), dim3(kFftThreads), specbank_lds_bytes(Fi), sb->st, a);
    }
    CSDR_HIP_TRY(hipGetLastError());
    return bank ? bank_iq_release(bank, sb->st) : CSDR_OK;
}

extern "C" int csdr_specbank_process(csdr_specbank *sb, const csdr_specbank_item *items, int n_items) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (int rc = sb_check_ready(sb)) return rc;
    bool any_dev = false;
    if (int rc = sb_check_items(items, n_items, sb->max_slots, &any_dev)) return rc;
    return sb_run(sb, items, n_items, any_dev);
}

extern "C" int csdr_specbank_process_bank(csdr_specbank *sb, csdr_bank *bank) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (int rc = sb_check_ready(sb)) return rc;
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

extern "C" int csdr_specbank_frames(const csdr_specbank *sb, int slot) { return sb_frames(sb, slot); }

extern "C" int csdr_specbank_fetch(csdr_specbank *sb, int slot, int frame, float *points_host, int cap_floats, double *fft_ceiling, double *fft_floor) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    return sb_fetch(sb, slot, frame, points_host, cap_floats, fft_ceiling, fft_floor);
}

extern "C" int csdr_specbank_fetch_hold(csdr_specbank *sb, int slot, int frame, float *hold_host, int cap_floats, int *n_floats) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    return sb_fetch_hold(sb, slot, frame, hold_host, cap_floats, n_floats);
}

extern "C" int csdr_specbank_device_points(csdr_specbank *sb, int slot, const float **dev, int *frames) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    return sb_device_points(sb, slot, dev, frames);
}

// ---- the points for a reader that stays on the device (csdr_objects.hpp) ----
int specbank_points_acquire(csdr_specbank *sb, hipStream_t reader, SpecBankPointsRef *out) {
    if (!sb || !sb->ready || !out) return fail(CSDR_ESTATE, "spectrum bank not set up");
    if (int rc = sb->points_gate.acquire(sb->st, reader)) return rc;
    out->ctx = sb->ctx; out->points = sb->points.p; out->F = sb->F; out->max_slots = sb->max_slots; out->max_frames = sb->max_frames;
    return CSDR_OK;
}
int specbank_points_release(csdr_specbank *sb, hipStream_t reader) { return sb->points_gate.release(reader); }
