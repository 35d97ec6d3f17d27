// DemodViews.h -- the zoomed demodulator spectrum per demodulator: N SpectrumVisualProcessors in setView(true, centre, bandwidth), fed the
// demodulators' CHANNEL rows as SDRPostThread hands them to IQActiveDemodVisualDataOutput (SDRPostThread.cpp:289-291, :334, :386), with the setters'
// names of the reference's src/process/SpectrumVisualProcessor.h; own implementation.  The reference shows this picture for the ACTIVE demodulator
// only (AppFrame.cpp:785-792, :2317-2320); a station that demodulates hundreds of channels on one device wants it for each.
//
// The bank is a csdr_viewbank (include/csdr_hip.h, "View bank"): state and points stay in HBM, and process(post, slots, channels) is ONE device
// call behind csdr_post_execute -- every slot and every block of the execute in one launch, no host synchronisation.  It NEEDS a context: the view
// branch runs every input through an msresamp_crcf, and a host-only arithmetic path would need a host msresamp, which this mirror does not carry
// (out of scope).  Without a context every call is refused with CSDR_ESTATE and logged.
#pragma once
#include <vector>

#include "HipPipeline.h"

class DemodViewBank {
public:
    // one process() input of a slot; n == 0: no input at all
    struct Item { int slot; const liquid_float_complex_t *data; int n; long long frequency; long long sampleRate; };

    explicit DemodViewBank(csdr_ctx *ctx) : ctx_(ctx) {
        if (ctx_) csdr_must(csdr_viewbank_create(ctx_, &vb_), "csdr_viewbank_create");
    }
    ~DemodViewBank() { if (vb_) csdr_viewbank_destroy(vb_); }
    DemodViewBank(const DemodViewBank &) = delete;
    DemodViewBank &operator=(const DemodViewBank &) = delete;
    bool onDevice() const { return vb_ != nullptr; }
    csdr_viewbank *handle() { return vb_; }
    CsdrErrorLog errlog;

    // setup(fftSize_in) (:140-178) for every slot; false: the size or the counts are refused (csdr_hip.h, "View bank", item 1)
    bool setup(unsigned int fftSize_in, int maxSlots, int maxFrames, int maxSamples) {
        if (!need("DemodViewBank::setup")) return false;
        if (!errlog.ok(csdr_viewbank_setup(vb_, (int)fftSize_in, maxSlots, maxFrames, maxSamples), "csdr_viewbank_setup")) return false;
        fftSize = fftSize_in;
        return true;
    }
    void setFFTAverageRate(float fftAverageRate) { if (need("DemodViewBank::setFFTAverageRate")) (void)errlog.ok(csdr_viewbank_set_average_rate(vb_, fftAverageRate), "csdr_viewbank_set_average_rate"); }
    void setScaleFactor(float sf) { if (need("DemodViewBank::setScaleFactor")) (void)errlog.ok(csdr_viewbank_set_scale_factor(vb_, sf), "csdr_viewbank_set_scale_factor"); }
    void setPeakHold(bool peakHold_in) { if (need("DemodViewBank::setPeakHold")) (void)errlog.ok(csdr_viewbank_set_peak_hold(vb_, peakHold_in ? 1 : 0), "csdr_viewbank_set_peak_hold"); }   // :115-125, on every slot
    bool getPeakHold() const { return vb_ && csdr_viewbank_get_peak_hold(vb_) != 0; }
    void setHideDC(bool hideDC) { if (need("DemodViewBank::setHideDC")) (void)errlog.ok(csdr_viewbank_set_hide_dc(vb_, hideDC ? 1 : 0), "csdr_viewbank_set_hide_dc"); }   // :204-209
    // setView(true, centerFreq_in, bandwidth_in) (:64-72) on one slot
    bool setView(int slot, long long centerFreq_in, long bandwidth_in) {
        return need("DemodViewBank::setView") && errlog.ok(csdr_viewbank_set_view(vb_, slot, centerFreq_in, bandwidth_in), "csdr_viewbank_set_view");
    }
    bool resetSlot(int slot) { return need("DemodViewBank::resetSlot") && errlog.ok(csdr_viewbank_reset_slot(vb_, slot), "csdr_viewbank_reset_slot"); }

    // slot slots[i] gets every block of row channels[i] of the post's last csdr_post_execute, where it lies in HBM, stamped with the row's centre
    // and the channel rate: ONE device call, no host synchronisation
    bool process(csdr_post *post, const std::vector<int> &slots, const std::vector<int> &channels) {
        if (!need("DemodViewBank::process")) return false;
        if (slots.size() != channels.size()) return errlog.ok(CSDR_EINVAL, "DemodViewBank::process");
        return errlog.ok(csdr_viewbank_process_post(vb_, post, slots.data(), channels.data(), (int)slots.size()), "csdr_viewbank_process_post");
    }
    // the items of one slot are its inputs in the order given; a refused call changes nothing
    bool process(const std::vector<Item> &items) {
        if (!need("DemodViewBank::process")) return false;
        std::vector<csdr_viewbank_item> it(items.size());
        for (size_t k = 0; k < items.size(); ++k)
            it[k] = csdr_viewbank_item{items[k].slot, items[k].n, items[k].data ? &items[k].data->real : nullptr, 0, 0, items[k].frequency, items[k].sampleRate};
        return errlog.ok(csdr_viewbank_process(vb_, it.data(), (int)it.size()), "csdr_viewbank_process");
    }
    int frames(int slot) const { return vb_ ? csdr_viewbank_frames(vb_, slot) : 0; }
    // SpectrumVisualData of a frame of the last process call (spectrum_hold_points empty when the frame carries none)
    bool fetch(int slot, int frame, SpectrumVisualData &out) {
        if (!need("DemodViewBank::fetch")) return false;
        out.spectrum_points.resize((size_t)fftSize * 2);
        out.spectrum_hold_points.resize((size_t)fftSize * 2);
        int nh = 0;
        if (!errlog.ok(csdr_viewbank_fetch(vb_, slot, frame, out.spectrum_points.data(), (int)out.spectrum_points.size(), &out.fft_ceiling, &out.fft_floor), "csdr_viewbank_fetch")) return false;
        if (!errlog.ok(csdr_viewbank_fetch_hold(vb_, slot, frame, out.spectrum_hold_points.data(), (int)out.spectrum_hold_points.size(), &nh), "csdr_viewbank_fetch_hold")) return false;
        out.spectrum_hold_points.resize((size_t)nh);
        return true;
    }
    bool slotInfo(int slot, csdr_viewbank_slot_state &out) { return need("DemodViewBank::slotInfo") && errlog.ok(csdr_viewbank_slot_info(vb_, slot, &out), "csdr_viewbank_slot_info"); }
    // a slot's lines of the last call into a waterfall panel of the same fft size, from where they lie (csdr_viewbank_device_points)
    bool stepInto(int slot, csdr_waterfall *wf) {
        if (!need("DemodViewBank::stepInto")) return false;
        const float *dev = nullptr;
        int n = 0;
        if (!errlog.ok(csdr_viewbank_device_points(vb_, slot, &dev, &n), "csdr_viewbank_device_points")) return false;
        return n == 0 || errlog.ok(csdr_waterfall_step(wf, dev, 1, (int)fftSize, n, nullptr), "csdr_waterfall_step");
    }

private:
    bool need(const char *what) { return vb_ ? true : errlog.ok(CSDR_ESTATE, what); }
    csdr_ctx *ctx_;
    csdr_viewbank *vb_ = nullptr;
    unsigned int fftSize = 0;
};
