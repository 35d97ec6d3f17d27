// csdr_viewbank.hip -- implementation of include/csdr_hip.h (gfx950): csdr_viewbank, N independent SpectrumVisualProcessors in zoomed view whose
// state and output stay in HBM.  The host plans every (slot, input) from its integers alone -- length, frequency, sample rate, the slot's view --
// exactly as the view branch of SpectrumVisualProcessor::process decides (:283-386): resampleBw and desiredInputSize, whether the retune is adopted
// and how far the averagers move, whether the resampler is rebuilt, num_written in closed form (design::resamp_count), the branch of the frame rule,
// where the peak-hold countdown stands.  ONE launch of viewbank_process (kernels_viewbank.hpp) does the arithmetic of all slots and all inputs of a
// call.  All work runs on a stream of the object's own; a channelizer's rows are reached through its batch events (csdr_viewbank_process_post).
#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <vector>

#define CSDR_TU_VIEWBANK 1     // this unit is the home of its kernel (kernels_viewbank.hpp)
#include "csdr_objects.hpp"
#include "kernels_viewbank.hpp"

using namespace csdr;

static_assert(sizeof(csdr_viewbank_item) == 40 && offsetof(csdr_viewbank_item, iq) == 8 && offsetof(csdr_viewbank_item, frequency) == 24, "csdr_viewbank_item layout");
static_assert(sizeof(csdr_viewbank_slot_state) == 32, "csdr_viewbank_slot_state layout");

namespace {
struct VbSlot {
    // setView (:64-72): survives csdr_viewbank_reset_slot
    bool has_view = false;
    int64_t centre = 0, bandwidth = 0;
    // the processor's integers
    int last_size = 0;                   // lastDataSize
    int peak_reset = 0;                  // peakReset
    int frames = 0;                      // frames of the last call
    long long last_bandwidth = 0, last_input_bandwidth = 0, shift_frequency = 0;
    bool have_resampler = false, last_view = false;
    int cfg = -1;                        // the resampler in force (csdr_viewbank::cfgs_h)
    uint32_t theta = 0, dtheta = 0;      // freqShifter: phase word, increment
    uint32_t buf_idx = 0, phase = 0;     // msresamp: buffer_index, the arbitrary stage's phase
    int64_t map_bw = 0, map_rbw = 0;     // (bandwidth, resampleBw) of the slot's map in HBM; 0, 0: none
    int map_new = -1;                    // planning: the map in force is the call's new_maps[map_new]; -1: the one in HBM
    // csdr_viewbank_slot_info
    int desired_input_size = 0, num_written = 0;
    int64_t resample_bw = 0;
};
constexpr int kVbPeakResetCount = 30;        // PEAK_RESET_COUNT (SpectrumVisualProcessor.h:12)
constexpr int kVbStage = 2;                  // page-locked staging sets of the plan
constexpr double kVbMaxBinsPerPoint = 64.0;  // a view wider than 32 input rates walks more bins per point than this: refused
}  // namespace

struct csdr_viewbank {
    csdr_ctx *ctx = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;      // boundary stream / channelizer -> st, st -> boundary stream (csdr_viewbank_device_points)
    bool ready = false;
    int F = 0, Fi = 0, max_slots = 0, max_frames = 0, max_samples = 0;
    float avg_rate = 0.65f, sf = 1.0f, sf_last = 1.0f;
    bool peak_hold = false, hide_dc = false;
    std::vector<VbSlot> slots;
    std::vector<int> touched;                          // slots that got frames in the last call
    DevBuf<float2> tw4096, last, stage, rs, y;
    DevBuf<double> ma, maa, peak;
    DevBuf<SpecBankTrk> trk;
    DevBuf<float> points, hold;
    DevBuf<SpecBankFrame> meta;
    DevBuf<int2> maps, maps_call;                      // [slots][F] the slots' view maps; the maps a call brings, until they are the slots'
    StageRing<kVbStage> plan;                          // SpecBankRun [runs] | ViewBankJob [jobs] of the call being run
    SpecBankTrk trk0{};
    // the resamplers designed so far, by the bit pattern of (float)resamplerRatio: a handful per input rate (resampleBw = rate / 2^k)
    std::map<uint32_t, int> cfg_index;
    std::vector<ResampCfg> cfgs_h;
    std::vector<float> arms_h;
    DevBuf<ResampCfg> cfgs_d;
    DevBuf<float> arms_d;
    size_t cfgs_on_device = 0;
    size_t lds_attr = 0;
    // scratch of a call's planning
    std::vector<VbSlot> work;
    std::vector<int> n_jobs_of, job_at, cursor, run_slots, job_map;
    std::vector<ViewBankJob> jobs_h;
    std::vector<std::pair<int, std::vector<int2>>> new_maps;
    std::vector<csdr_viewbank_item> post_items;
};

extern "C" int csdr_viewbank_create(csdr_ctx *ctx, csdr_viewbank **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    std::unique_ptr<csdr_viewbank> vb(new csdr_viewbank());
    vb->ctx = ctx;
    CSDR_HIP_TRY(hipStreamCreateWithFlags(&vb->st, hipStreamNonBlocking));
    CSDR_HIP_TRY(hipEventCreateWithFlags(&vb->ev_in, hipEventDisableTiming));
    CSDR_HIP_TRY(hipEventCreateWithFlags(&vb->ev_out, hipEventDisableTiming));
    if (int rc = vb->plan.create()) return rc;
    vb->trk0.ceil_ma = vb->trk0.ceil_maa = 100.0;       // ctor :32
    vb->trk0.floor_ma = vb->trk0.floor_maa = 0.0;       // ctor :33
    vb->trk0.ceil_peak = vb->trk0.floor_peak = 0.0;
    *out = vb.release();
    return CSDR_OK;
}

extern "C" void csdr_viewbank_destroy(csdr_viewbank *vb) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (!vb) return;
    if (vb->st) { (void)hipStreamSynchronize(vb->st); (void)hipStreamDestroy(vb->st); }
    if (vb->ev_in) (void)hipEventDestroy(vb->ev_in);
    if (vb->ev_out) (void)hipEventDestroy(vb->ev_out);
    vb->plan.destroy();
    vb->tw4096.release(); vb->last.release(); vb->stage.release(); vb->rs.release(); vb->y.release(); vb->ma.release(); vb->maa.release();
    vb->peak.release(); vb->trk.release(); vb->points.release(); vb->hold.release(); vb->meta.release(); vb->maps.release(); vb->maps_call.release();
    vb->cfgs_d.release(); vb->arms_d.release();
    delete vb;
}

// a slot as SpectrumVisualProcessor's constructor and setup(fftSize_in) leave it, with setPeakHold(the object's setting) and the slot's last
// setView called once.  (The resampler's windows in HBM need no fill: the first input builds a resampler, and a new resampler starts empty.)
static int vb_reset_slot(csdr_viewbank *vb, int slot) {
    const size_t Fi = (size_t)vb->Fi, o = (size_t)slot * Fi;
    CSDR_HIP_TRY(hipMemsetAsync(vb->last.p + o, 0, Fi * sizeof(float2), vb->st));
    CSDR_HIP_TRY(hipMemsetAsync(vb->ma.p + o, 0, Fi * sizeof(double), vb->st));
    CSDR_HIP_TRY(hipMemsetAsync(vb->maa.p + o, 0, Fi * sizeof(double), vb->st));
    CSDR_HIP_TRY(hipMemsetAsync(vb->peak.p + o, 0, Fi * sizeof(double), vb->st));
    CSDR_HIP_TRY(hipMemcpyAsync(vb->trk.p + slot, &vb->trk0, sizeof(SpecBankTrk), hipMemcpyHostToDevice, vb->st));
    VbSlot &s = vb->slots[(size_t)slot];
    VbSlot fresh;
    fresh.has_view = s.has_view; fresh.centre = s.centre; fresh.bandwidth = s.bandwidth;
    fresh.peak_reset = 1;                                // setPeakHold :115-125 on a processor whose peakHold was false
    s = fresh;
    return CSDR_OK;
}

extern "C" int csdr_viewbank_setup(csdr_viewbank *vb, int fft_size, int max_slots, int max_frames, int max_samples) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (!vb) return fail(CSDR_EINVAL, "view bank is null");
    if (fft_size < 8) return fail(CSDR_EINVAL, "fft_size %d: a power of two, 8 .. %d", fft_size, kFftMaxLds / 2);
    if ((fft_size & (fft_size - 1)) != 0 || fft_size > kFftMaxLds / 2) return fail(CSDR_EUNSUPPORTED, "fft_size %d: a power of two, 8 .. %d", fft_size, kFftMaxLds / 2);
    if (max_slots < 1 || max_slots > 4096) return fail(CSDR_EINVAL, "max_slots %d: 1 .. 4096", max_slots);
    if (max_frames < 1) return fail(CSDR_EINVAL, "max_frames %d", max_frames);
    if (max_samples < 1) return fail(CSDR_EINVAL, "max_samples %d", max_samples);
    CSDR_HIP_TRY(hipStreamSynchronize(vb->st));
    vb->ready = false;
    const size_t Fi = 2 * (size_t)fft_size, S = (size_t)max_slots;        // SPECTRUM_VZM (.h:11, :145)
    if (!vb->tw4096.p) {
        std::vector<float2> t(kTwTab);
        for (int i = 0; i < kTwTab; i++) { const double a = -2.0 * M_PI * i / kTwTab; t[(size_t)i] = make_float2((float)std::cos(a), (float)std::sin(a)); }
        if (int rc = vb->tw4096.reserve(kTwTab)) return rc;
        CSDR_HIP_TRY(hipMemcpy(vb->tw4096.p, t.data(), kTwTab * sizeof(float2), hipMemcpyHostToDevice));
    }
    if (int rc = vb->last.reserve(S * Fi)) return rc;
    if (int rc = vb->y.reserve(S * Fi)) return rc;
    if (int rc = vb->rs.reserve(S * (size_t)kVbState)) return rc;
    if (int rc = vb->ma.reserve(S * Fi)) return rc;
    if (int rc = vb->maa.reserve(S * Fi)) return rc;
    if (int rc = vb->peak.reserve(S * Fi)) return rc;
    if (int rc = vb->trk.reserve(S)) return rc;
    if (int rc = vb->maps.reserve(S * (size_t)fft_size)) return rc;
    if (int rc = vb->points.reserve(S * (size_t)max_frames * (size_t)fft_size)) return rc;
    if (int rc = vb->hold.reserve(S * (size_t)max_frames * (size_t)fft_size)) return rc;
    if (int rc = vb->meta.reserve(S * (size_t)max_frames)) return rc;
    // setup makes every slot a processor nobody has called setView on
    vb->F = fft_size; vb->Fi = (int)Fi; vb->max_slots = max_slots; vb->max_frames = max_frames; vb->max_samples = max_samples;
    vb->slots.assign(S, VbSlot());
    vb->touched.clear();
    CSDR_HIP_TRY(hipMemsetAsync(vb->last.p, 0, S * Fi * sizeof(float2), vb->st));
    CSDR_HIP_TRY(hipMemsetAsync(vb->y.p, 0, S * Fi * sizeof(float2), vb->st));
    CSDR_HIP_TRY(hipMemsetAsync(vb->rs.p, 0, S * (size_t)kVbState * sizeof(float2), vb->st));
    CSDR_HIP_TRY(hipMemsetAsync(vb->ma.p, 0, S * Fi * sizeof(double), vb->st));
    CSDR_HIP_TRY(hipMemsetAsync(vb->maa.p, 0, S * Fi * sizeof(double), vb->st));
    CSDR_HIP_TRY(hipMemsetAsync(vb->peak.p, 0, S * Fi * sizeof(double), vb->st));
    std::vector<SpecBankTrk> t0(S, vb->trk0);
    CSDR_HIP_TRY(hipMemcpyAsync(vb->trk.p, t0.data(), S * sizeof(SpecBankTrk), hipMemcpyHostToDevice, vb->st));
    CSDR_HIP_TRY(hipStreamSynchronize(vb->st));          // (t0 is this call's)
    for (VbSlot &s : vb->slots) s.peak_reset = 1;
    vb->ready = true;
    return CSDR_OK;
}

extern "C" int csdr_viewbank_set_average_rate(csdr_viewbank *vb, float rate) {     // setFFTAverageRate
    if (!vb) return fail(CSDR_EINVAL, "view bank is null");
    vb->avg_rate = rate;
    return CSDR_OK;
}
extern "C" int csdr_viewbank_set_scale_factor(csdr_viewbank *vb, float sf) {       // setScaleFactor
    if (!vb) return fail(CSDR_EINVAL, "view bank is null");
    vb->sf = sf;
    return CSDR_OK;
}
extern "C" int csdr_viewbank_set_peak_hold(csdr_viewbank *vb, int enabled) {       // setPeakHold :115-125, on every slot
    if (!vb) return fail(CSDR_EINVAL, "view bank is null");
    const bool again = vb->peak_hold && enabled;
    for (VbSlot &s : vb->slots) s.peak_reset = again ? kVbPeakResetCount : 1;
    if (!again) vb->peak_hold = enabled != 0;
    return CSDR_OK;
}
extern "C" int csdr_viewbank_get_peak_hold(const csdr_viewbank *vb) { return vb && vb->peak_hold ? 1 : 0; }
extern "C" int csdr_viewbank_set_hide_dc(csdr_viewbank *vb, int enabled) {         // setHideDC :204-209
    if (!vb) return fail(CSDR_EINVAL, "view bank is null");
    vb->hide_dc = enabled != 0;
    return CSDR_OK;
}

extern "C" int csdr_viewbank_set_view(csdr_viewbank *vb, int slot, int64_t center_freq, int64_t bandwidth) {     // setView(true, ...) :64-72
    if (!vb || !vb->ready) return fail(CSDR_ESTATE, "view bank not set up");
    if (slot < 0 || slot >= vb->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, vb->max_slots);
    if (bandwidth <= 0) return fail(CSDR_EINVAL, "bandwidth %lld", (long long)bandwidth);
    VbSlot &s = vb->slots[(size_t)slot];
    s.has_view = true; s.centre = center_freq; s.bandwidth = bandwidth;
    return CSDR_OK;
}

extern "C" int csdr_viewbank_reset_slot(csdr_viewbank *vb, int slot) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (!vb || !vb->ready) return fail(CSDR_ESTATE, "view bank not set up");
    if (slot < 0 || slot >= vb->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, vb->max_slots);
    return vb_reset_slot(vb, slot);
}

// the resampler of (float)resamplerRatio (:361: msresamp_crcf_create(resamplerRatio, 60)): designed once per ratio, on the host
static int vb_cfg_for(csdr_viewbank *vb, float ratio) {
    uint32_t key;
    memcpy(&key, &ratio, sizeof key);
    auto it = vb->cfg_index.find(key);
    if (it != vb->cfg_index.end()) return it->second;
    const design::MsresampPlan p = design::plan_msresamp(ratio, 60.0f);
    const int idx = (int)vb->cfgs_h.size();
    ResampCfg rc;
    if (p.S <= (unsigned)kMaxHb && !p.interp) fill_resamp_cfg(rc, p, idx);
    else { memset(&rc, 0, sizeof rc); rc.S = (int)p.S; rc.interp = p.interp ? 1 : 0; }      // (never run: the call that asks for it is refused)
    vb->cfgs_h.push_back(rc);
    vb->arms_h.insert(vb->arms_h.end(), p.arms.begin(), p.arms.end());
    vb->cfg_index[key] = idx;
    return idx;
}

// the bin walk of :532-560 for visualRatio = bandwidth / resampleBw, stepped with the reference's own accumulator: (first bin, bins) per point
static void vb_view_map(int F, int64_t bandwidth, int64_t resample_bw, std::vector<int2> &vm) {
    const int N = 2 * F;
    vm.resize((size_t)F);
    const double visualRatio = double(bandwidth) / double(resample_bw);
    const double visualStart = (double(N) / 2.0) - (double(N) * (visualRatio / 2.0));
    double visualAccum = 0, i = 0;
    for (int x = 0; x < F; ++x) {
        visualAccum += visualRatio * 2.0;
        long long first = 0;
        int cnt = 0;
        while (visualAccum >= 1.0) {
            if (!cnt) first = (long long)std::round(visualStart + i);        // (a negative index wraps far beyond Fi as unsigned: not inside either way)
            ++cnt; visualAccum -= 1.0; i += 1.0;
        }
        vm[(size_t)x] = make_int2((int)first, cnt);
    }
}

// the plan and the launch of one call; `items` are checked.  any_dev: an input lies in device memory the caller produced on the boundary stream;
// post: the inputs are rows of that channelizer's last batch -- waited for and handed back by events once the call can no longer be refused
static int vb_run(csdr_viewbank *vb, const csdr_viewbank_item *items, int n_items, bool any_dev, csdr_post *post = nullptr) {
    const int Fi = vb->Fi, F = vb->F;
    // ---- plan on copies: a refused call leaves every slot as it was
    vb->n_jobs_of.assign((size_t)vb->max_slots, 0);
    size_t n_jobs = 0;
    for (int i = 0; i < n_items; ++i) {
        const csdr_viewbank_item &it = items[i];
        if (it.n == 0) continue;                          // no input at all
        if (!vb->slots[(size_t)it.slot].has_view) return fail(CSDR_ESTATE, "item %d: slot %d was never given a view", i, it.slot);
        if (it.n > vb->max_samples) return fail(CSDR_ERANGE, "item %d: %d samples exceed max_samples %d", i, it.n, vb->max_samples);
        ++vb->n_jobs_of[(size_t)it.slot];
        ++n_jobs;
    }
    vb->run_slots.clear();
    vb->job_at.assign((size_t)vb->max_slots, 0);
    vb->work.resize((size_t)vb->max_slots);
    {
        int at = 0;
        for (int s = 0; s < vb->max_slots; ++s)
            if (vb->n_jobs_of[(size_t)s]) {
                vb->run_slots.push_back(s); vb->job_at[(size_t)s] = at; at += vb->n_jobs_of[(size_t)s];
                vb->work[(size_t)s] = vb->slots[(size_t)s];
                vb->work[(size_t)s].frames = 0;
                vb->work[(size_t)s].map_new = -1;
            }
    }
    vb->jobs_h.resize(n_jobs);
    vb->job_map.assign(n_jobs, -1);
    vb->new_maps.clear();
    vb->cursor = vb->job_at;
    size_t host_samples = 0;
    int S_max = 0;
    for (int i = 0; i < n_items; ++i) {
        const csdr_viewbank_item &it = items[i];
        if (it.n == 0) continue;
        VbSlot &s = vb->work[(size_t)it.slot];
        const size_t ji = (size_t)vb->cursor[(size_t)it.slot]++;
        ViewBankJob jb{};
        jb.frame = -1;
        jb.do_peak = vb->peak_hold && s.peak_reset == 0 ? 1 : 0;              // :247
        if (s.peak_reset != 0 && --s.peak_reset == 0) jb.peak_reset_now = 1;  // :264-273
        const long long rate = it.sample_rate, freq = it.frequency;
        if (rate < 0) return fail(CSDR_EINVAL, "item %d: sample rate %lld", i, rate);
        if (rate == 0) {                                                      // :284-287
            jb.action = kVbNone;
            s.last_view = true;
            vb->jobs_h[ji] = jb;
            continue;
        }
        long long rbw = rate;
        while (rbw / 2 >= s.bandwidth && rbw / 2 > 0) rbw /= 2;               // :289-291 (long division)
        const double ratio = (double)rbw / (double)rate;                      // :293
        size_t desired = (size_t)((double)Fi / ratio);                        // :295
        s.desired_input_size = (int)desired;
        s.resample_bw = rbw;
        if ((size_t)it.n < desired) desired = (size_t)it.n;                   // :297-302
        if ((double)s.bandwidth / (double)rbw * 2.0 > kVbMaxBinsPerPoint)
            return fail(CSDR_EUNSUPPORTED, "item %d: a view of %lld Hz on an input of %lld Hz walks more than %d bins per point", i, (long long)s.bandwidth, rate, (int)kVbMaxBinsPerPoint);
        const bool mix = s.centre != freq;                                    // :304
        if (mix && ((s.centre - freq) != s.shift_frequency || s.last_input_bandwidth != rate)) {
            if (std::llabs(freq - s.centre) < rate / 2) {                     // :306 (the application rate is the input's)
                const long long last_shift = s.shift_frequency;
                s.shift_frequency = s.centre - freq;
                s.dtheta = design::nco_phase_word((float)((2.0 * M_PI) * (((double)std::llabs(s.shift_frequency)) / ((double)rate))));      // :311
                const long long freq_diff = s.shift_frequency - last_shift;
                if (s.last_bandwidth != 0) {                                  // :316-331
                    const double bin_per_hz = double(s.last_bandwidth) / double(Fi);
                    const double ns = std::floor(double(std::llabs(freq_diff)) / bin_per_hz);
                    if (ns > 0.0 && ns < (double)(Fi / 2)) { jb.shift_mode = freq_diff > 0 ? kVbLeft : kVbRight; jb.shift_n = (int)ns; }
                }
            }
            s.peak_reset = kVbPeakResetCount;                                 // :335
        }
        bool new_resampler = false;
        long long bw_diff = 0;
        if (!s.have_resampler || rbw != s.last_bandwidth || s.last_input_bandwidth != rate) {      // :354-368
            s.cfg = vb_cfg_for(vb, (float)ratio);
            const ResampCfg &rc = vb->cfgs_h[(size_t)s.cfg];
            if (rc.S > kMaxHb || rc.interp) return fail(CSDR_EUNSUPPORTED, "item %d: a view of %lld Hz on an input of %lld Hz needs %d half-band stages (limit %d)", i, (long long)s.bandwidth, rate, rc.S, kMaxHb);
            bw_diff = rbw - s.last_bandwidth;
            s.last_bandwidth = rbw; s.last_input_bandwidth = rate;
            s.have_resampler = true;
            s.buf_idx = 0; s.phase = 0;
            new_resampler = true;
            jb.rebuild = 1;
            s.peak_reset = kVbPeakResetCount;                                 // :367
        }
        const ResampCfg &rc = vb->cfgs_h[(size_t)s.cfg];
        S_max = std::max(S_max, rc.S);
        jb.cfg = s.cfg;
        jb.n = (int)desired;
        jb.theta0 = s.theta; jb.dtheta = s.dtheta;
        jb.mixdir = !mix ? 0 : (s.shift_frequency < 0 ? +1 : -1);             // :345-351
        if (mix) s.theta += (uint32_t)desired * s.dtheta;
        jb.buf0 = (int)s.buf_idx; jb.phase0 = s.phase;
        const uint64_t groups = ((uint64_t)s.buf_idx + desired) >> rc.S;
        uint32_t phase_after = 0;
        const int nw = (int)design::resamp_count(groups, s.phase, rc.step, &phase_after);      // num_written
        s.phase = phase_after;
        s.buf_idx = (uint32_t)(((uint64_t)s.buf_idx + desired) & (((uint64_t)1 << rc.S) - 1));
        jb.nw = nw;
        s.num_written = nw;
        // the frame rule of :399-421 on num_written
        if (nw >= Fi) { jb.action = kSbFull; jb.arg = 0; }
        else if (s.last_size + nw < Fi) {
            jb.action = kSbPrime;
            jb.arg = std::max(Fi - s.last_size, nw);
            s.last_size += jb.arg;
        } else {
            if (s.last_size > Fi) return fail(CSDR_ESTATE, "slot %d: lastDataSize %d beyond %d", it.slot, s.last_size, Fi);      // (cannot happen: priming stops at Fi)
            jb.action = kSbSlide;
            jb.arg = s.last_size - (Fi - nw);
        }
        if (jb.action != kSbPrime) {
            jb.frame = s.frames++;
            if (new_resampler && s.last_view) jb.rescale = bw_diff < 0 ? kVbSqueeze : kVbStretch;      // :454
            if (s.map_bw != s.bandwidth || s.map_rbw != rbw) {
                vb->new_maps.emplace_back(it.slot, std::vector<int2>());
                vb_view_map(F, s.bandwidth, rbw, vb->new_maps.back().second);
                s.map_new = (int)vb->new_maps.size() - 1;
                s.map_bw = s.bandwidth; s.map_rbw = rbw;
            }
            vb->job_map[ji] = s.map_new;
            if (vb->hide_dc) {
                const HideDcSpan d = hide_dc_span(s.centre, freq, (long)s.bandwidth, F);
                jb.dc_start = d.start; jb.dc_half = d.half; jb.dc_end = d.end;
            }
        }
        s.last_view = true;                                                   // :631
        jb.src = it.is_dev ? reinterpret_cast<const float2 *>(it.iq) : nullptr;       // (a host input: its place in the staging buffer, below)
        if (!it.is_dev) host_samples += (size_t)jb.n;
        vb->jobs_h[ji] = jb;
    }
    for (int s : vb->run_slots)
        if (vb->work[(size_t)s].frames > vb->max_frames)
            return fail(CSDR_ERANGE, "slot %d: %d frames in one call exceed max_frames %d", s, vb->work[(size_t)s].frames, vb->max_frames);
    // ---- commit the host state; from here on the call is enqueued
    for (int s : vb->touched) vb->slots[(size_t)s].frames = 0;
    vb->touched = vb->run_slots;
    for (int s : vb->run_slots) { vb->slots[(size_t)s] = vb->work[(size_t)s]; vb->slots[(size_t)s].map_new = -1; }
    vb->sf_last = vb->sf;
    if (n_jobs == 0) return CSDR_OK;
    hipStream_t st = vb->st;
    if (post) {      // the rows of the channelizer's batch are complete
        const int pk = post->cur;
        csdr_ctx *c = post->ctx;
        if (c->same(LANE_POST, LANE_FE)) { CSDR_HIP_TRY(hipEventRecord(vb->ev_in, c->lanes[LANE_POST])); CSDR_HIP_TRY(hipStreamWaitEvent(st, vb->ev_in, 0)); }    // (ev_ready is recorded only between two streams)
        else CSDR_HIP_TRY(hipStreamWaitEvent(st, post->ev_ready[pk], 0));
    }
    if (any_dev) {
        CSDR_HIP_TRY(hipEventRecord(vb->ev_in, vb->ctx->stream));
        CSDR_HIP_TRY(hipStreamWaitEvent(st, vb->ev_in, 0));
    }
    // resamplers designed since the last upload
    if (vb->cfgs_on_device < vb->cfgs_h.size()) {
        const size_t n = vb->cfgs_h.size(), per = (size_t)kArms * kArmTaps;
        size_t from = vb->cfgs_on_device;
        if (n > vb->cfgs_d.cap) {
            CSDR_HIP_TRY(hipStreamSynchronize(st));                           // (a kernel may still read the tables being replaced)
            const size_t cap = std::max<size_t>(8, 2 * n);
            if (int rc = vb->cfgs_d.reserve(cap)) return rc;
            if (int rc = vb->arms_d.reserve(cap * per)) return rc;
            from = 0;
        }
        CSDR_HIP_TRY(hipMemcpyAsync(vb->cfgs_d.p + from, vb->cfgs_h.data() + from, (n - from) * sizeof(ResampCfg), hipMemcpyHostToDevice, st));
        CSDR_HIP_TRY(hipMemcpyAsync(vb->arms_d.p + from * per, vb->arms_h.data() + from * per, (n - from) * per * sizeof(float), hipMemcpyHostToDevice, st));
        vb->cfgs_on_device = n;
    }
    // the maps this call brings: jobs read them where they are uploaded; behind the kernel each slot's latest becomes the slot's
    if (!vb->new_maps.empty()) {
        const size_t need = vb->new_maps.size() * (size_t)F;
        if (need > vb->maps_call.cap) CSDR_HIP_TRY(hipStreamSynchronize(st));
        if (int rc = vb->maps_call.reserve(need)) return rc;
        for (size_t k = 0; k < vb->new_maps.size(); ++k)
            CSDR_HIP_TRY(hipMemcpyAsync(vb->maps_call.p + k * (size_t)F, vb->new_maps[k].second.data(), (size_t)F * sizeof(int2), hipMemcpyHostToDevice, st));
    }
    for (size_t r = 0; r < vb->run_slots.size(); ++r) {
        const int s = vb->run_slots[r];
        for (int k = 0; k < vb->n_jobs_of[(size_t)s]; ++k) {
            const size_t ji = (size_t)vb->job_at[(size_t)s] + (size_t)k;
            const int mi = vb->job_map[ji];
            vb->jobs_h[ji].map = mi < 0 ? vb->maps.p + (size_t)s * (size_t)F : vb->maps_call.p + (size_t)mi * (size_t)F;
        }
    }
    if (host_samples) {
        if (host_samples > vb->stage.cap) CSDR_HIP_TRY(hipStreamSynchronize(st));        // (a kernel may still read the buffer being replaced)
        if (int rc = vb->stage.reserve(host_samples)) return rc;
        size_t at = 0;
        vb->cursor = vb->job_at;
        for (int i = 0; i < n_items; ++i) {                // host inputs, staged in item order: the samples the input consumes
            const csdr_viewbank_item &it = items[i];
            if (it.n == 0) continue;
            ViewBankJob &jb = vb->jobs_h[(size_t)vb->cursor[(size_t)it.slot]++];
            if (it.is_dev || jb.action == kVbNone) continue;
            float2 *dst = vb->stage.p + at;
            CSDR_HIP_TRY(hipMemcpyAsync(dst, it.iq, (size_t)jb.n * sizeof(float2), hipMemcpyHostToDevice, st));
            jb.src = dst;
            at += (size_t)jb.n;
        }
    }
    const size_t n_runs = vb->run_slots.size();
    const size_t bytes = n_runs * sizeof(SpecBankRun) + n_jobs * sizeof(ViewBankJob);
    if (int rc = vb->plan.begin(st, bytes)) return rc;               // the one host wait of a call
    SpecBankRun *runs_h = reinterpret_cast<SpecBankRun *>(vb->plan.host());
    for (size_t r = 0; r < n_runs; ++r) {
        const int s = vb->run_slots[r];
        runs_h[r] = SpecBankRun{s, vb->job_at[(size_t)s], vb->n_jobs_of[(size_t)s], 0};
    }
    memcpy(vb->plan.host() + n_runs * sizeof(SpecBankRun), vb->jobs_h.data(), n_jobs * sizeof(ViewBankJob));
    if (int rc = vb->plan.uploaded(st, bytes)) return rc;
    ViewBankArgs a{};
    a.runs = reinterpret_cast<const SpecBankRun *>(vb->plan.device());
    a.jobs = reinterpret_cast<const ViewBankJob *>(vb->plan.device() + n_runs * sizeof(SpecBankRun));
    a.tw4096 = vb->tw4096.p; a.sintab = vb->ctx->sintab.p; a.cfgs = vb->cfgs_d.p; a.arms = vb->arms_d.p;
    a.last = vb->last.p; a.ma = vb->ma.p; a.maa = vb->maa.p; a.peak = vb->peak.p; a.trk = vb->trk.p; a.rs = vb->rs.p; a.y = vb->y.p;
    a.points = vb->points.p; a.hold = vb->hold.p; a.meta = vb->meta.p;
    a.Fi = Fi; a.max_frames = vb->max_frames; a.rate = (double)vb->avg_rate; a.sf = vb->sf;
    const size_t lds = viewbank_lds_bytes(Fi, S_max);
    if (lds > 64 * 1024 && lds > vb->lds_attr) {
        CSDR_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(viewbank_process), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        vb->lds_attr = lds;
    }
    {
        ProfScope ps__(vb->ctx, KID_VIEWBANK, st);
        hipLaunchKernelGGL(viewbank_process, dim3((unsigned)n_runs), dim3(kFftThreads), lds, st, a);
    }
    CSDR_HIP_TRY(hipGetLastError());
    {   // each slot's latest map of this call becomes the slot's, behind the kernel that may still read the previous one
        std::vector<int> &latest = vb->cursor;
        latest.assign((size_t)vb->max_slots, -1);
        for (size_t k = 0; k < vb->new_maps.size(); ++k) latest[(size_t)vb->new_maps[k].first] = (int)k;
        for (size_t k = 0; k < vb->new_maps.size(); ++k) {
            const int s = vb->new_maps[k].first;
            if (latest[(size_t)s] != (int)k) continue;
            CSDR_HIP_TRY(hipMemcpyAsync(vb->maps.p + (size_t)s * (size_t)F, vb->maps_call.p + k * (size_t)F, (size_t)F * sizeof(int2), hipMemcpyDeviceToDevice, st));
        }
    }
    if (post) {      // the channelizer rewrites this batch's buffer only behind the kernel
        const int pk = post->cur;
        post->rotate = true;
        CSDR_HIP_TRY(hipEventRecord(post->ev_consumed[pk][post->n_consumed[pk]++], st));
    }
    return CSDR_OK;
}

extern "C" int csdr_viewbank_process(csdr_viewbank *vb, const csdr_viewbank_item *items, int n_items) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (!vb || !vb->ready) return fail(CSDR_ESTATE, "view bank not set up");
    if (n_items < 0 || (n_items > 0 && !items)) return fail(CSDR_EINVAL, "bad items");
    bool any_dev = false;
    for (int i = 0; i < n_items; ++i) {
        const csdr_viewbank_item &it = items[i];
        if (it.slot < 0 || it.slot >= vb->max_slots) return fail(CSDR_EINVAL, "item %d: slot %d of %d", i, it.slot, vb->max_slots);
        if (it.n < 0 || (it.n > 0 && !it.iq)) return fail(CSDR_EINVAL, "item %d: %d samples at %p", i, it.n, (const void *)it.iq);
        if (it.n > 0 && it.is_dev) {
            if ((uintptr_t)it.iq & 7) return fail(CSDR_EINVAL, "item %d: device samples must be 8-byte aligned", i);
            any_dev = true;
        }
    }
    return vb_run(vb, items, n_items, any_dev);
}

extern "C" int csdr_viewbank_process_post(csdr_viewbank *vb, csdr_post *post, const int *slots, const int *channels, int n) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (!vb || !vb->ready) return fail(CSDR_ESTATE, "view bank not set up");
    if (!post || n < 0 || (n > 0 && (!slots || !channels))) return fail(CSDR_EINVAL, "bad argument");
    if (post->ctx != vb->ctx) return fail(CSDR_EINVAL, "the channelizer belongs to another context");
    if (!post->row_order.empty()) return fail(CSDR_EINVAL, "the post has packed rows (a time-slab producer): views read the owner's post");
    if (!post->configured || post->n_blocks <= 0 || post->seq == 0) return fail(CSDR_ESTATE, "no csdr_post_execute yet");
    const int NB = post->n_blocks, M = post->M, Bc = post->block_len / post->hop;
    const int64_t rate = csdr_post_channel_rate(post);
    vb->post_items.clear();
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= vb->max_slots) return fail(CSDR_EINVAL, "entry %d: slot %d of %d", i, slots[i], vb->max_slots);
        const int ch = channels[i];
        if (ch < 0 || ch >= M) return fail(CSDR_EINVAL, "entry %d: channel %d of %d", i, ch, M);
        if (M > 1 && !std::binary_search(post->active_host.begin(), post->active_host.end(), ch))
            return fail(CSDR_EINVAL, "entry %d: channel %d is not produced by the channelizer", i, ch);
        const int64_t centre = M == 1 ? post->frequency : post->centers[(size_t)ch];
        const float2 *row = post_buf(post, post->cur) + (int64_t)ch * post->chan_stride;
        for (int bb = 0; bb < NB; ++bb)
            vb->post_items.push_back(csdr_viewbank_item{slots[i], Bc, reinterpret_cast<const float *>(row + (size_t)bb * Bc), 1, 0, centre, rate});
    }
    if (vb->post_items.empty()) return vb_run(vb, nullptr, 0, false);
    if (post->n_consumed[post->cur] >= csdr_post::kMaxConsumers) return fail(CSDR_ERANGE, "too many readers of one channelizer batch");
    return vb_run(vb, vb->post_items.data(), (int)vb->post_items.size(), false, post);
}

extern "C" int csdr_viewbank_frames(const csdr_viewbank *vb, int slot) {
    return vb && vb->ready && slot >= 0 && slot < vb->max_slots ? vb->slots[(size_t)slot].frames : 0;
}

static int vb_check_frame(const csdr_viewbank *vb, int slot, int frame) {
    if (!vb || !vb->ready) return fail(CSDR_ESTATE, "view bank not set up");
    if (slot < 0 || slot >= vb->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, vb->max_slots);
    if (frame < 0 || frame >= vb->slots[(size_t)slot].frames) return fail(CSDR_EINVAL, "frame %d of %d", frame, vb->slots[(size_t)slot].frames);
    return CSDR_OK;
}

// SpectrumVisualData of a frame: the device keeps only the y of every point; the x of point i is (float)i / (float)fftSize (:563)
static int vb_fetch(csdr_viewbank *vb, const float *src, size_t fo, float *host, SpecBankFrame *m) {
    const int F = vb->F;
    CSDR_HIP_TRY(hipMemcpyAsync(host + F, src + fo * (size_t)F, (size_t)F * sizeof(float), hipMemcpyDeviceToHost, vb->st));
    CSDR_HIP_TRY(hipMemcpyAsync(m, vb->meta.p + fo, sizeof(SpecBankFrame), hipMemcpyDeviceToHost, vb->st));
    CSDR_HIP_TRY(hipStreamSynchronize(vb->st));
    for (int i = 0; i < F; ++i) { const float y = host[F + i]; host[2 * i] = (float)i / (float)F; host[2 * i + 1] = y; }
    return CSDR_OK;
}

extern "C" int csdr_viewbank_fetch(csdr_viewbank *vb, int slot, int frame, float *points_host, int cap_floats, double *fft_ceiling, double *fft_floor) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (int rc = vb_check_frame(vb, slot, frame)) return rc;
    if (!points_host) return fail(CSDR_EINVAL, "null argument");
    if (cap_floats < 2 * vb->F) return fail(CSDR_ERANGE, "need room for %d floats", 2 * vb->F);
    SpecBankFrame m{};
    const size_t fo = (size_t)slot * (size_t)vb->max_frames + (size_t)frame;
    if (int rc = vb_fetch(vb, vb->points.p, fo, points_host, &m)) return rc;
    if (fft_ceiling) *fft_ceiling = m.point_ceil / vb->sf_last;          // :626
    if (fft_floor) *fft_floor = m.point_floor;                           // :627
    return CSDR_OK;
}

extern "C" int csdr_viewbank_fetch_hold(csdr_viewbank *vb, int slot, int frame, float *hold_host, int cap_floats, int *n_floats) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (n_floats) *n_floats = 0;
    if (int rc = vb_check_frame(vb, slot, frame)) return rc;
    if (!hold_host || !n_floats) return fail(CSDR_EINVAL, "null argument");
    if (cap_floats < 2 * vb->F) return fail(CSDR_ERANGE, "need room for %d floats", 2 * vb->F);
    SpecBankFrame m{};
    const size_t fo = (size_t)slot * (size_t)vb->max_frames + (size_t)frame;
    if (int rc = vb_fetch(vb, vb->hold.p, fo, hold_host, &m)) return rc;
    *n_floats = m.hold ? 2 * vb->F : 0;
    return CSDR_OK;
}

extern "C" int csdr_viewbank_device_points(csdr_viewbank *vb, int slot, const float **dev, int *frames) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (!vb || !vb->ready) return fail(CSDR_ESTATE, "view bank not set up");
    if (!dev || slot < 0 || slot >= vb->max_slots) return fail(CSDR_EINVAL, "bad argument");
    CSDR_HIP_TRY(hipEventRecord(vb->ev_out, vb->st));     // whatever the caller enqueues on the boundary stream next reads the finished points
    CSDR_HIP_TRY(hipStreamWaitEvent(vb->ctx->stream, vb->ev_out, 0));
    *dev = vb->points.p + (size_t)slot * (size_t)vb->max_frames * (size_t)vb->F;
    if (frames) *frames = vb->slots[(size_t)slot].frames;
    return CSDR_OK;
}

extern "C" int csdr_viewbank_slot_info(const csdr_viewbank *vb, int slot, csdr_viewbank_slot_state *out) {
    if (!vb || !vb->ready) return fail(CSDR_ESTATE, "view bank not set up");
    if (!out || slot < 0 || slot >= vb->max_slots) return fail(CSDR_EINVAL, "bad argument");
    const VbSlot &s = vb->slots[(size_t)slot];
    out->resample_bw = s.resample_bw; out->shift_frequency = s.shift_frequency;
    out->desired_input_size = s.desired_input_size; out->last_data_size = s.last_size; out->peak_reset = s.peak_reset; out->num_written = s.num_written;
    return CSDR_OK;
}

extern "C" int csdr_viewbank_fetch_last(csdr_viewbank *vb, int slot, float *out, int cap_floats) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (!vb || !vb->ready) return fail(CSDR_ESTATE, "view bank not set up");
    if (!out || slot < 0 || slot >= vb->max_slots) return fail(CSDR_EINVAL, "bad argument");
    if (cap_floats < 2 * vb->Fi) return fail(CSDR_ERANGE, "need room for %d floats", 2 * vb->Fi);
    CSDR_HIP_TRY(hipMemcpyAsync(out, vb->last.p + (size_t)slot * (size_t)vb->Fi, (size_t)vb->Fi * sizeof(float2), hipMemcpyDeviceToHost, vb->st));
    CSDR_HIP_TRY(hipStreamSynchronize(vb->st));
    return CSDR_OK;
}
