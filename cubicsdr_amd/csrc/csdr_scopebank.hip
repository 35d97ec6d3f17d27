// csdr_scopebank.hip -- implementation of include/csdr_hip.h (gfx950): csdr_scopebank, N independent ScopeVisualProcessors whose state and items stay
// in HBM.  The host plans every (slot, frame) of a call -- the job records per slot, outSize per frame by the float arithmetic of
// ScopeVisualProcessor.cpp:194-200 -- and uploads the plan, with the samples of host frames behind it, from page-locked staging sets in rotation; ONE
// launch of scopebank_wave and ONE of scopebank_spectrum (kernels_scopebank.hpp) do the arithmetic of all slots and all frames of a call.  All work
// runs on a stream of the object's own, as the spectrum bank's does; the demodulator bank's audio and scope taps are reached through
// bank_audio_acquire / _release (csdr_objects.hpp), ordered by events.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#define CSDR_TU_SCOPEBANK 1     // this unit is the home of its kernels (kernels_scopebank.hpp)
#include "csdr_objects.hpp"
#include "kernels_scopebank.hpp"

using namespace csdr;

static_assert(sizeof(csdr_scopebank_item) == 56 && offsetof(csdr_scopebank_item, frame) == 8, "csdr_scopebank_item layout");

namespace {
constexpr int kScbStage = 2;                 // page-locked staging sets of the plan
}  // namespace

struct csdr_scopebank : SideStream, SlotOrder {         // (ev_in: device frames of the caller; ev_out: csdr_scopebank_device_points; the slot order of a call)
    bool ready = false, scope_on = true, spectrum_on = true;           // ctor :8-9
    int L = 0, max_slots = 0, max_frames = 0, max_n = 0, max_scope_samples = 1024;      // maxScopeSamples = DEFAULT_DMOD_FFT_SIZE (:13)
    float rate = 0.65f;                                // fft_average_rate (:10)
    bool last_wave = false, last_spec = false;         // which halves the last call produced
    std::vector<int> frames;                           // per slot: frames of the last call
    DevBuf<float2> tw4096;
    DevBuf<double> ma, maa;
    DevBuf<ScopeTrk> trk;
    DevBuf<float> wave_pts, spec_pts;
    DevBuf<ScopeMeta> wave_meta, spec_meta;
    StageRing<kScbStage> plan;                         // ScopeBankRun [runs] | ScopeBankJob [jobs] | float [samples of the host frames] of the call being run
    std::vector<ScopeBankJob> jobs_h;                  // scratch of a call's planning
    std::vector<csdr_scopebank_item> bank_items;
};

extern "C" int csdr_scopebank_create(csdr_ctx *ctx, csdr_scopebank **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    std::unique_ptr<csdr_scopebank, void (*)(csdr_scopebank *)> sb(new csdr_scopebank(), csdr_scopebank_destroy);
    if (int rc = sb->create(ctx)) return rc;
    if (int rc = sb->plan.create()) return rc;
    *out = sb.release();
    return CSDR_OK;
}

extern "C" void csdr_scopebank_destroy(csdr_scopebank *sb) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb) return;
    sb->destroy();
    sb->plan.destroy();
    sb->tw4096.release(); sb->ma.release(); sb->maa.release(); sb->trk.release();
    sb->wave_pts.release(); sb->spec_pts.release(); sb->wave_meta.release(); sb->spec_meta.release();
    delete sb;
}

// a slot as ScopeVisualProcessor's constructor and setup(fftSize_in) leave it (:8-13, :24-35): averagers (vector::resize, :158-162) and trackers zero
static int scb_reset_slot(csdr_scopebank *sb, int slot) {
    const size_t H = (size_t)sb->L / 2, o = (size_t)slot * H;
    CSDR_HIP_TRY(hipMemsetAsync(sb->ma.p + o, 0, H * sizeof(double), sb->st));
    CSDR_HIP_TRY(hipMemsetAsync(sb->maa.p + o, 0, H * sizeof(double), sb->st));
    CSDR_HIP_TRY(hipMemsetAsync(sb->trk.p + slot, 0, sizeof(ScopeTrk), sb->st));
    sb->frames[(size_t)slot] = 0;
    return CSDR_OK;
}

extern "C" int csdr_scopebank_setup(csdr_scopebank *sb, int fft_size, int max_slots, int max_frames, int max_samples) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb) return fail(CSDR_EINVAL, "scope bank is null");
    // the sizes csdr_scope_setup takes: the in-LDS transform holds fft_size <= 4096 points
    if (fft_size < 4 || (fft_size & (fft_size - 1)) != 0 || fft_size > kFftMaxLds) return fail(CSDR_EUNSUPPORTED, "scope fft size %d: powers of two, 4 .. %d", fft_size, kFftMaxLds);
    if (max_slots < 1 || max_slots > 4096) return fail(CSDR_EINVAL, "max_slots %d: 1 .. 4096", max_slots);
    if (max_frames < 1 || max_samples < 1) return fail(CSDR_EINVAL, "max_frames %d, max_samples %d", max_frames, max_samples);
    CSDR_HIP_TRY(hipStreamSynchronize(sb->st));
    sb->ready = false;
    const size_t H = (size_t)fft_size / 2, S = (size_t)max_slots, SF = S * (size_t)max_frames;
    if (int rc = upload_twiddles(sb->tw4096, kTwTab)) return rc;
    if (int rc = sb->ma.reserve(S * H)) return rc;
    if (int rc = sb->maa.reserve(S * H)) return rc;
    if (int rc = sb->trk.reserve(S)) return rc;
    if (int rc = sb->wave_pts.reserve(SF * 2 * (size_t)max_samples)) return rc;
    if (int rc = sb->spec_pts.reserve(SF * (size_t)fft_size)) return rc;
    if (int rc = sb->wave_meta.reserve(SF)) return rc;
    if (int rc = sb->spec_meta.reserve(SF)) return rc;
    sb->L = fft_size; sb->max_slots = max_slots; sb->max_frames = max_frames; sb->max_n = max_samples;
    sb->frames.assign(S, 0);
    sb->touched.clear();
    sb->last_wave = sb->last_spec = false;
    // every slot a fresh processor: one fill per array
    CSDR_HIP_TRY(hipMemsetAsync(sb->ma.p, 0, S * H * sizeof(double), sb->st));
    CSDR_HIP_TRY(hipMemsetAsync(sb->maa.p, 0, S * H * sizeof(double), sb->st));
    CSDR_HIP_TRY(hipMemsetAsync(sb->trk.p, 0, S * sizeof(ScopeTrk), sb->st));
    // the spectrum kernel's two L-point arrays + its reduction scratch pass the 64 KB default at fftSize 4096
    if (scopebank_lds_bytes(fft_size) > 64 * 1024)
        CSDR_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(scopebank_spectrum), hipFuncAttributeMaxDynamicSharedMemorySize, (int)scopebank_lds_bytes(fft_size)));
    sb->ready = true;
    return CSDR_OK;
}

extern "C" int csdr_scopebank_set_enabled(csdr_scopebank *sb, int scope_on, int spectrum_on) {     // setScopeEnabled / setSpectrumEnabled :37-43, on every slot
    if (!sb) return fail(CSDR_EINVAL, "scope bank is null");
    sb->scope_on = scope_on != 0; sb->spectrum_on = spectrum_on != 0;
    return CSDR_OK;
}
extern "C" int csdr_scopebank_set_max_scope_samples(csdr_scopebank *sb, int n) {
    if (!sb || n <= 0) return fail(CSDR_EINVAL, "bad argument");
    sb->max_scope_samples = n;
    return CSDR_OK;
}
extern "C" int csdr_scopebank_set_average_rate(csdr_scopebank *sb, float rate) {
    if (!sb) return fail(CSDR_EINVAL, "scope bank is null");
    sb->rate = rate;
    return CSDR_OK;
}

extern "C" int csdr_scopebank_reset_slot(csdr_scopebank *sb, int slot) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb || !sb->ready) return fail(CSDR_ESTATE, "scope bank not set up");
    if (slot < 0 || slot >= sb->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, sb->max_slots);
    return scb_reset_slot(sb, slot);
}

static bool scb_empty(const csdr_scopebank_item &it) { return it.frame.n == 0 || it.frame.data == nullptr; }     // no input at all (:53-61)

// every check of a call, in front of anything that is enqueued or changed: the whole call is refused or none of it
static int scb_check(csdr_scopebank *sb, const csdr_scopebank_item *items, int n_items) {
    sb->count_begin(sb->max_slots);
    for (int i = 0; i < n_items; ++i) {
        const csdr_scopebank_item &it = items[i];
        const csdr_scope_frame &f = it.frame;
        if (it.slot < 0 || it.slot >= sb->max_slots) return fail(CSDR_EINVAL, "item %d: slot %d of %d", i, it.slot, sb->max_slots);
        if (scb_empty(it)) continue;
        if (f.n < 0) return fail(CSDR_EINVAL, "item %d: %d samples", i, f.n);
        if (f.channels != 1 && f.channels != 2) return fail(CSDR_EINVAL, "item %d: %d channels", i, f.channels);
        if (f.layout < 0 || f.layout > 2) return fail(CSDR_EINVAL, "item %d: layout %d", i, f.layout);
        if (f.n > sb->max_n) return fail(CSDR_ERANGE, "item %d: %d samples exceed max_samples %d", i, f.n, sb->max_n);
        sb->count_job(it.slot);
    }
    for (int s = 0; s < sb->max_slots; ++s)
        if (sb->n_jobs_of[(size_t)s] > sb->max_frames)
            return fail(CSDR_ERANGE, "slot %d: %d frames in one call exceed max_frames %d", s, sb->n_jobs_of[(size_t)s], sb->max_frames);
    return CSDR_OK;
}

// the plan and the two launches of one call; `items` passed scb_check (which counted the jobs per slot).  data_is_dev: the frames lie in device memory the
// caller produced on the boundary stream; bank: they are that bank's audio / scope taps -- acquired here, where the call can no longer be refused,
// released behind the kernels
static int scb_run(csdr_scopebank *sb, const csdr_scopebank_item *items, int n_items, bool data_is_dev, csdr_bank *bank = nullptr) {
    const size_t n_jobs = sb->order();
    size_t host_floats = 0;
    if (!data_is_dev)
        for (int i = 0; i < n_items; ++i) if (!scb_empty(items[i])) host_floats += (size_t)items[i].frame.n;
    // ---- commit the host state; from here on the call is enqueued
    sb->commit([&](int s) { sb->frames[(size_t)s] = 0; }, [&](int s) { sb->frames[(size_t)s] = sb->n_jobs_of[(size_t)s]; });
    sb->last_wave = sb->scope_on; sb->last_spec = sb->spectrum_on;
    if (n_jobs == 0 || (!sb->scope_on && !sb->spectrum_on)) return CSDR_OK;
    if (bank) { if (int rc = bank_audio_acquire(bank, sb->st)) return rc; }
    else if (data_is_dev) { if (int rc = sb->after_boundary()) return rc; }
    const size_t n_runs = sb->run_slots.size();
    const size_t off_jobs = sb->run_bytes(), off_data = off_jobs + n_jobs * sizeof(ScopeBankJob);
    const size_t bytes = off_data + host_floats * sizeof(float);
    if (int rc = sb->plan.begin(sb->st, bytes)) return rc;           // the one host wait of a call
    sb->fill_runs(sb->plan.host());
    sb->jobs_h.resize(n_jobs);
    float *data_h = reinterpret_cast<float *>(sb->plan.host() + off_data);
    const float *data_d = reinterpret_cast<const float *>(sb->plan.device() + off_data);
    size_t at = 0;
    for (int i = 0; i < n_items; ++i) {
        const csdr_scopebank_item &it = items[i];
        if (scb_empty(it)) continue;
        const csdr_scope_frame &f = it.frame;
        const int j = (int)sb->next_job(it.slot);
        ScopeBankJob &jb = sb->jobs_h[(size_t)j];
        memset(&jb, 0, sizeof jb);
        ScopeFrame &d = jb.fr;
        d.data = f.data; d.n_dev = data_is_dev ? f.n_dev : nullptr; d.n = f.n; d.channels = f.channels; d.type = f.type; d.layout = f.layout;
        d.scale = f.layout ? f.scale : 1.0f;
        d.sample_rate = f.sample_rate; d.input_rate = f.input_rate; d.pad = 0;
        // spectrum points kept: fftSize / 2, scaled down when the tap runs below the rate it is labelled with (:194-200, float arithmetic)
        unsigned out_size = (unsigned)sb->L / 2;
        if (f.sample_rate != f.input_rate) out_size = (unsigned)(int)std::floor((float)out_size * ((float)f.sample_rate / (float)f.input_rate));
        d.out_size = (int)std::min<unsigned>(out_size, (unsigned)sb->L / 2);
        if (!data_is_dev) {                               // a host frame: its samples ride behind the plan
            memcpy(data_h + at, f.data, (size_t)f.n * sizeof(float));
            d.data = data_d + at;
            at += (size_t)f.n;
        }
        jb.slot = it.slot;
        jb.frame = j - sb->job_at[(size_t)it.slot];
    }
    memcpy(sb->plan.host() + off_jobs, sb->jobs_h.data(), n_jobs * sizeof(ScopeBankJob));
    if (int rc = sb->plan.uploaded(sb->st, bytes)) return rc;
    ScopeBankArgs a{};
    a.runs = reinterpret_cast<const ScopeBankRun *>(sb->plan.device());
    a.jobs = reinterpret_cast<const ScopeBankJob *>(sb->plan.device() + off_jobs);
    a.tw4096 = sb->tw4096.p;
    a.ma = sb->ma.p; a.maa = sb->maa.p; a.trk = sb->trk.p;
    a.wave_pts = sb->wave_pts.p; a.spec_pts = sb->spec_pts.p; a.wave_meta = sb->wave_meta.p; a.spec_meta = sb->spec_meta.p;
    a.L = sb->L; a.max_frames = sb->max_frames; a.max_n = sb->max_n; a.max_scope_samples = sb->max_scope_samples;
    a.rate = (double)sb->rate;
    if (sb->scope_on) {
        ProfScope ps__(sb->ctx, KID_SCOPEBANK_WAVE, sb->st);
        hipLaunchKernelGGL(scopebank_wave, dim3((unsigned)n_jobs), dim3(kScopeThreads), 64, sb->st, a);
    }
    if (sb->spectrum_on) {
        ProfScope ps__(sb->ctx, KID_SCOPEBANK_SPECTRUM, sb->st);
        hipLaunchKernelGGL(scopebank_spectrum, dim3((unsigned)n_runs), dim3(kFftThreads), scopebank_lds_bytes(sb->L), sb->st, a);
    }
    CSDR_HIP_TRY(hipGetLastError());
    return bank ? bank_audio_release(bank, sb->st) : CSDR_OK;
}

extern "C" int csdr_scopebank_process(csdr_scopebank *sb, const csdr_scopebank_item *items, int n_items, int data_is_dev) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb || !sb->ready) return fail(CSDR_ESTATE, "scope bank not set up");
    if (n_items < 0 || (n_items > 0 && !items)) return fail(CSDR_EINVAL, "bad items");
    if (int rc = scb_check(sb, items, n_items)) return rc;
    return scb_run(sb, items, n_items, data_is_dev != 0);
}

extern "C" int csdr_scopebank_process_bank(csdr_scopebank *sb, csdr_bank *bank) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb || !sb->ready) return fail(CSDR_ESTATE, "scope bank not set up");
    if (!bank) return fail(CSDR_EINVAL, "bank is null");
    if (bank->ctx != sb->ctx) return fail(CSDR_EINVAL, "the bank belongs to another context");
    if (bank->last_nb == 0) return fail(CSDR_ESTATE, "no csdr_bank_execute yet");
    // one item for every configured, active slot the object has room for: the tap of the last block of the last execute, where it lies in HBM; a block
    // the front-end skipped, a front-end-only, host or digital slot has nothing to show (n = 0): no input
    sb->bank_items.clear();
    const int ns = std::min(sb->max_slots, bank->max_demods);
    for (int si = 0; si < ns; ++si) {
        const SlotHost &s = bank->slots[(size_t)si];
        if (!s.configured || !s.active) continue;
        csdr_scopebank_item it{};
        it.slot = si;
        if (int rc = csdr_bank_scope_frame(bank, si, &it.frame)) return rc;
        if (!scb_empty(it)) sb->bank_items.push_back(it);
    }
    if (int rc = scb_check(sb, sb->bank_items.data(), (int)sb->bank_items.size())) return rc;
    return scb_run(sb, sb->bank_items.data(), (int)sb->bank_items.size(), true, sb->bank_items.empty() ? nullptr : bank);
}

extern "C" int csdr_scopebank_frames(const csdr_scopebank *sb, int slot) {
    return sb && sb->ready && slot >= 0 && slot < sb->max_slots ? sb->frames[(size_t)slot] : 0;
}

// item of frame `frame` of the slot's last process: which = 0 the waveform (ScopeRenderData with spectrum == false), 1 the spectrum.
// info->n_floats == 0 when that half was switched off.
extern "C" int csdr_scopebank_fetch(csdr_scopebank *sb, int slot, int frame, int which, float *points, int cap_floats, csdr_scope_info *info) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb || !sb->ready) return fail(CSDR_ESTATE, "scope bank not set up");
    if (!points || !info) return fail(CSDR_EINVAL, "null argument");
    if (slot < 0 || slot >= sb->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, sb->max_slots);
    if (frame < 0 || frame >= sb->frames[(size_t)slot] || which < 0 || which > 1) return fail(CSDR_EINVAL, "frame %d of %d", frame, sb->frames[(size_t)slot]);
    memset(info, 0, sizeof *info);
    if ((which == 0 && !sb->last_wave) || (which == 1 && !sb->last_spec)) return CSDR_OK;
    const size_t fo = (size_t)slot * (size_t)sb->max_frames + (size_t)frame;
    ScopeMeta m;
    CSDR_HIP_TRY(hipMemcpyAsync(&m, (which ? sb->spec_meta.p : sb->wave_meta.p) + fo, sizeof m, hipMemcpyDeviceToHost, sb->st));
    CSDR_HIP_TRY(hipStreamSynchronize(sb->st));
    if (m.n_floats > cap_floats) return fail(CSDR_ERANGE, "need %d floats", m.n_floats);
    const float *src = which ? sb->spec_pts.p + fo * (size_t)sb->L : sb->wave_pts.p + fo * 2 * (size_t)sb->max_n;
    if (m.n_floats > 0) {
        CSDR_HIP_TRY(hipMemcpyAsync(points, src, (size_t)m.n_floats * sizeof(float), hipMemcpyDeviceToHost, sb->st));
        CSDR_HIP_TRY(hipStreamSynchronize(sb->st));
    }
    info->mode = m.mode; info->spectrum = m.spectrum; info->channels = m.channels; info->input_rate = m.input_rate; info->sample_rate = m.sample_rate;
    info->fft_size = m.fft_size; info->n_floats = m.n_floats; info->fft_floor = m.fft_floor; info->fft_ceil = m.fft_ceil;
    return CSDR_OK;
}

extern "C" int csdr_scopebank_device_points(csdr_scopebank *sb, int slot, int which, const float **dev, int *frames, int *stride_floats) {
    DeviceScope dev__(sb ? sb->ctx : nullptr);
    if (!sb || !sb->ready) return fail(CSDR_ESTATE, "scope bank not set up");
    if (!dev || slot < 0 || slot >= sb->max_slots || which < 0 || which > 1) return fail(CSDR_EINVAL, "bad argument");
    if (int rc = sb->hand_over()) return rc;              // whatever the caller enqueues on the boundary stream next reads the finished items
    const size_t fo = (size_t)slot * (size_t)sb->max_frames;
    const int stride = which ? sb->L : 2 * sb->max_n;
    *dev = (which ? sb->spec_pts.p : sb->wave_pts.p) + fo * (size_t)stride;
    if (frames) *frames = (which ? sb->last_spec : sb->last_wave) ? sb->frames[(size_t)slot] : 0;
    if (stride_floats) *stride_floats = stride;
    return CSDR_OK;
}
