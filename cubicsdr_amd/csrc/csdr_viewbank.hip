// csdr_viewbank.hip -- implementation of include/csdr_hip.h (gfx950): csdr_viewbank, N independent SpectrumVisualProcessors in zoomed view whose
// state and output stay in HBM.  The host plans every (slot, input) from its integers alone -- length, frequency, sample rate, the slot's view --
// exactly as the view branch of SpectrumVisualProcessor::process decides (:283-386): resampleBw and desiredInputSize, whether the retune is adopted
// and how far the averagers move, whether the resampler is rebuilt, num_written in closed form (design::resamp_count), the branch of the frame rule,
// where the peak-hold countdown stands.  ONE launch of viewbank_process (kernels_viewbank.hpp) does the arithmetic of all slots and all inputs of a
// call.  All work runs on a stream of the object's own; a channelizer's rows are reached through its batch events (csdr_viewbank_process_post).
// The frame store, the countdown, the frame rule, the slot order of a call and the fetches are specbank_host.hpp's, shared with csdr_specbank.hip;
// this unit states the view plan, the resamplers and maps, and where the inputs come from.
#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <vector>

#define CSDR_TU_VIEWBANK 1     // this unit is the home of its kernel (kernels_viewbank.hpp)
#include "specbank_host.hpp"
#include "kernels_viewbank.hpp"

using namespace csdr;

static_assert(sizeof(csdr_viewbank_item) == 40 && offsetof(csdr_viewbank_item, iq) == 8 && offsetof(csdr_viewbank_item, frequency) == 24, "csdr_viewbank_item layout");
static_assert(sizeof(csdr_viewbank_slot_state) == 32, "csdr_viewbank_slot_state layout");

namespace {
struct VbSlot : SbSlot {
    // setView (:64-72): survives csdr_viewbank_reset_slot
    bool has_view = false;
    int64_t centre = 0, bandwidth = 0;
    // the processor's integers (lastDataSize, peakReset and the frames of the last call: SbSlot)
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
constexpr double kVbMaxBinsPerPoint = 64.0;  // a view wider than 32 input rates walks more bins per point than this: refused
}  // namespace

struct csdr_viewbank : SbBank<VbSlot, ViewBankJob> {
    static constexpr const char *kName = "view bank";
    int max_samples = 0;
    bool hide_dc = false;
    DevBuf<float2> rs, y;
    DevBuf<int2> maps, maps_call;                      // [slots][F] the slots' view maps; the maps a call brings, until they are the slots'
    // the resamplers designed so far, by the bit pattern of (float)resamplerRatio: a handful per input rate (resampleBw = rate / 2^k)
    std::map<uint32_t, int> cfg_index;
    std::vector<ResampCfg> cfgs_h;
    std::vector<float> arms_h;
    DevBuf<ResampCfg> cfgs_d;
    DevBuf<float> arms_d;
    size_t cfgs_on_device = 0;
    size_t lds_attr = 0;
    // scratch of a call's planning
    std::vector<int> job_map;
    std::vector<std::pair<int, std::vector<int2>>> new_maps;
    std::vector<csdr_viewbank_item> post_items;
};

extern "C" int csdr_viewbank_create(csdr_ctx *ctx, csdr_viewbank **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    std::unique_ptr<csdr_viewbank, void (*)(csdr_viewbank *)> vb(new csdr_viewbank(), csdr_viewbank_destroy);
    if (int rc = vb->create_base(ctx)) return rc;
    *out = vb.release();
    return CSDR_OK;
}

extern "C" void csdr_viewbank_destroy(csdr_viewbank *vb) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (!vb) return;
    vb->destroy_base();
    vb->rs.release(); vb->y.release(); vb->maps.release(); vb->maps_call.release(); vb->cfgs_d.release(); vb->arms_d.release();
    delete vb;
}

// a slot as SpectrumVisualProcessor's constructor and setup(fftSize_in) leave it, with setPeakHold(the object's setting) and the slot's last
// setView called once.  (The resampler's windows in HBM need no fill: the first input builds a resampler, and a new resampler starts empty.)
static int vb_reset_slot(csdr_viewbank *vb, int slot) {
    if (int rc = vb->reset_frames(slot)) return rc;
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
    if (int rc = sb_check_setup(fft_size, max_slots, max_frames)) return rc;
    if (max_samples < 1) return fail(CSDR_EINVAL, "max_samples %d", max_samples);
    CSDR_HIP_TRY(hipStreamSynchronize(vb->st));
    vb->ready = false;
    if (int rc = vb->reserve_frames(fft_size, max_slots, max_frames)) return rc;
    const size_t Fi = (size_t)vb->Fi, S = (size_t)max_slots;
    if (int rc = vb->y.reserve(S * Fi)) return rc;
    if (int rc = vb->rs.reserve(S * (size_t)kVbState)) return rc;
    if (int rc = vb->maps.reserve(S * (size_t)fft_size)) return rc;
    vb->max_samples = max_samples;
    CSDR_HIP_TRY(hipMemsetAsync(vb->y.p, 0, S * Fi * sizeof(float2), vb->st));
    CSDR_HIP_TRY(hipMemsetAsync(vb->rs.p, 0, S * (size_t)kVbState * sizeof(float2), vb->st));
    if (int rc = vb->fresh_slots()) return rc;            // every slot a processor nobody has called setView on (ends in a synchronise)
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
extern "C" int csdr_viewbank_set_peak_hold(csdr_viewbank *vb, int enabled) {
    if (!vb) return fail(CSDR_EINVAL, "view bank is null");
    vb->set_peak_hold(enabled);
    return CSDR_OK;
}
extern "C" int csdr_viewbank_get_peak_hold(const csdr_viewbank *vb) { return vb && vb->peak_hold ? 1 : 0; }
extern "C" int csdr_viewbank_set_hide_dc(csdr_viewbank *vb, int enabled) {         // setHideDC :204-209
    if (!vb) return fail(CSDR_EINVAL, "view bank is null");
    vb->hide_dc = enabled != 0;
    return CSDR_OK;
}

extern "C" int csdr_viewbank_set_view(csdr_viewbank *vb, int slot, int64_t center_freq, int64_t bandwidth) {     // setView(true, ...) :64-72
    if (int rc = sb_check_slot(vb, slot)) return rc;
    if (bandwidth <= 0) return fail(CSDR_EINVAL, "bandwidth %lld", (long long)bandwidth);
    VbSlot &s = vb->slots[(size_t)slot];
    s.has_view = true; s.centre = center_freq; s.bandwidth = bandwidth;
    return CSDR_OK;
}

extern "C" int csdr_viewbank_reset_slot(csdr_viewbank *vb, int slot) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (int rc = sb_check_slot(vb, slot)) return rc;
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
    vb->count_begin(vb->max_slots);
    size_t n_jobs = 0;
    for (int i = 0; i < n_items; ++i) {
        const csdr_viewbank_item &it = items[i];
        if (it.n == 0) continue;                          // no input at all
        if (!vb->slots[(size_t)it.slot].has_view) return fail(CSDR_ESTATE, "item %d: slot %d was never given a view", i, it.slot);
        if (it.n > vb->max_samples) return fail(CSDR_ERANGE, "item %d: %d samples exceed max_samples %d", i, it.n, vb->max_samples);
        vb->count_job(it.slot);
        ++n_jobs;
    }
    vb->order_jobs();
    vb->job_map.assign(n_jobs, -1);
    vb->new_maps.clear();
    size_t host_samples = 0;
    int S_max = 0;
    for (int i = 0; i < n_items; ++i) {
        const csdr_viewbank_item &it = items[i];
        if (it.n == 0) continue;
        VbSlot &s = vb->work[(size_t)it.slot];
        const size_t ji = vb->next_job(it.slot);
        ViewBankJob jb{};
        jb.frame = -1;
        vb->job_head(jb, s);
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
            s.peak_reset = kSbPeakResetCount;                                 // :335
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
            s.peak_reset = kSbPeakResetCount;                                 // :367
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
        if (int rc = vb->frame_rule(jb, s, it.slot, nw)) return rc;           // :399-421 on num_written
        if (jb.action != kSbPrime) {
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
    if (int rc = vb->check_frames()) return rc;
    vb->commit();
    for (int s : vb->run_slots) vb->slots[(size_t)s].map_new = -1;
    if (n_jobs == 0) return CSDR_OK;
    hipStream_t st = vb->st;
    if (post) {      // the rows of the channelizer's batch are complete
        const int pk = post->cur;
        csdr_ctx *c = post->ctx;
        if (c->same(LANE_POST, LANE_FE)) { if (int rc = vb->after(c->lanes[LANE_POST])) return rc; }    // (ev_ready is recorded only between two streams)
        else CSDR_HIP_TRY(hipStreamWaitEvent(st, post->ev_ready[pk], 0));
    }
    if (any_dev) if (int rc = vb->after_boundary()) return rc;
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
    if (int rc = vb->stage_inputs(items, n_items, host_samples)) return rc;
    ViewBankArgs a{};
    if (int rc = vb->upload_plan(&a.runs, &a.jobs)) return rc;
    vb->fill_args(a);
    a.sintab = vb->ctx->sintab.p; a.cfgs = vb->cfgs_d.p; a.arms = vb->arms_d.p; a.rs = vb->rs.p; a.y = vb->y.p;
    const size_t lds = viewbank_lds_bytes(Fi, S_max);
    if (lds > 64 * 1024 && lds > vb->lds_attr) {
        CSDR_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(viewbank_process), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        vb->lds_attr = lds;
    }
    {
        ProfScope ps__(vb->ctx, KID_VIEWBANK, st);
        hipLaunchKernelGGL(viewbank_process, dim3((unsigned)vb->run_slots.size()), dim3(kFftThreads), lds, st, a);
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
    if (int rc = sb_check_ready(vb)) return rc;
    bool any_dev = false;
    if (int rc = sb_check_items(items, n_items, vb->max_slots, &any_dev)) return rc;
    return vb_run(vb, items, n_items, any_dev);
}

extern "C" int csdr_viewbank_process_post(csdr_viewbank *vb, csdr_post *post, const int *slots, const int *channels, int n) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (int rc = sb_check_ready(vb)) return rc;
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

extern "C" int csdr_viewbank_frames(const csdr_viewbank *vb, int slot) { return sb_frames(vb, slot); }

extern "C" int csdr_viewbank_fetch(csdr_viewbank *vb, int slot, int frame, float *points_host, int cap_floats, double *fft_ceiling, double *fft_floor) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    return sb_fetch(vb, slot, frame, points_host, cap_floats, fft_ceiling, fft_floor);
}

extern "C" int csdr_viewbank_fetch_hold(csdr_viewbank *vb, int slot, int frame, float *hold_host, int cap_floats, int *n_floats) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    return sb_fetch_hold(vb, slot, frame, hold_host, cap_floats, n_floats);
}

extern "C" int csdr_viewbank_device_points(csdr_viewbank *vb, int slot, const float **dev, int *frames) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    return sb_device_points(vb, slot, dev, frames);
}

extern "C" int csdr_viewbank_slot_info(const csdr_viewbank *vb, int slot, csdr_viewbank_slot_state *out) {
    if (int rc = sb_check_ready(vb)) return rc;
    if (!out || slot < 0 || slot >= vb->max_slots) return fail(CSDR_EINVAL, "bad argument");
    const VbSlot &s = vb->slots[(size_t)slot];
    out->resample_bw = s.resample_bw; out->shift_frequency = s.shift_frequency;
    out->desired_input_size = s.desired_input_size; out->last_data_size = s.last_size; out->peak_reset = s.peak_reset; out->num_written = s.num_written;
    return CSDR_OK;
}

extern "C" int csdr_viewbank_fetch_last(csdr_viewbank *vb, int slot, float *out, int cap_floats) {
    DeviceScope dev__(vb ? vb->ctx : nullptr);
    if (int rc = sb_check_ready(vb)) return rc;
    if (!out || slot < 0 || slot >= vb->max_slots) return fail(CSDR_EINVAL, "bad argument");
    if (cap_floats < 2 * vb->Fi) return fail(CSDR_ERANGE, "need room for %d floats", 2 * vb->Fi);
    CSDR_HIP_TRY(hipMemcpyAsync(out, vb->last.p + (size_t)slot * (size_t)vb->Fi, (size_t)vb->Fi * sizeof(float2), hipMemcpyDeviceToHost, vb->st));
    CSDR_HIP_TRY(hipStreamSynchronize(vb->st));
    return CSDR_OK;
}
