// DemodScopes.h -- an audio scope per demodulator: N ScopeVisualProcessors of one fft size, with the setter names of the reference's
// src/process/ScopeVisualProcessor.h applied to all slots; own implementation.  The reference feeds this processor from the ACTIVE demodulator's audio
// tap only (DemodulatorThread.cpp:240-316); a station that monitors hundreds of channels on one device wants one behind each.
//
// The bank is a csdr_scopebank (include/csdr_hip.h, "Scope bank"): every slot's averagers, trackers and items stay in HBM, and process() is ONE device
// call -- the taps are read where the demodulators left them.  As ScopeVisualProcessor.h, the mirror has no host arithmetic: without a context the
// constructor throws.
#pragma once
#include <vector>

#include "HipPipeline.h"
#include "ScopeVisualProcessor.h"

class DemodScopeBank {
public:
    explicit DemodScopeBank(csdr_ctx *ctx) { csdr_must(csdr_scopebank_create(ctx, &sb_), "csdr_scopebank_create"); }
    ~DemodScopeBank() { if (sb_) csdr_scopebank_destroy(sb_); }
    DemodScopeBank(const DemodScopeBank &) = delete;
    DemodScopeBank &operator=(const DemodScopeBank &) = delete;
    csdr_scopebank *handle() { return sb_; }
    CsdrErrorLog errlog;

    // setup(fftSize_in) (:24-35) on every slot; one frame per slot and call, at most 2 * DEMOD_VIS_SIZE floats (the stereo tap,
    // DemodulatorThread.cpp:271-275).  false: a size or a count is refused (csdr_hip.h, "Scope bank", item 1)
    bool setup(int fftSize_in, int maxSlots) {
        if (!errlog.ok(csdr_scopebank_setup(sb_, fftSize_in, maxSlots, 1, kMaxFrameFloats), "csdr_scopebank_setup")) return false;
        fftSize_ = fftSize_in;
        return true;
    }
    void setScopeEnabled(bool on) { scopeOn_ = on; pushEnables(); }                     // :37-43, on every slot
    void setSpectrumEnabled(bool on) { spectrumOn_ = on; pushEnables(); }
    bool resetSlot(int slot) { return errlog.ok(csdr_scopebank_reset_slot(sb_, slot), "csdr_scopebank_reset_slot"); }

    // the scope tap of every active demodulator of the bank's last execute, HBM to HBM in one call
    bool process(csdr_bank *bank) { return errlog.ok(csdr_scopebank_process_bank(sb_, bank), "csdr_scopebank_process_bank"); }
    int frames(int slot) const { return csdr_scopebank_frames(sb_, slot); }
    // the item of a slot's frame: which = 0 the waveform, 1 the spectrum.  No points: that half is switched off, or there is no such frame (logged)
    ScopeRenderData item(int slot, int frame, int which) {
        ScopeRenderData out;
        out.waveform_points.resize((size_t)std::max(2 * kMaxFrameFloats, fftSize_));
        csdr_scope_info info{};
        if (!errlog.ok(csdr_scopebank_fetch(sb_, slot, frame, which, out.waveform_points.data(), (int)out.waveform_points.size(), &info), "csdr_scopebank_fetch")) info.n_floats = 0;
        out.waveform_points.resize((size_t)info.n_floats);
        if (info.n_floats == 0) return out;
        out.mode = (ScopePanel::ScopeMode)info.mode; out.spectrum = info.spectrum != 0;
        out.channels = info.channels; out.inputRate = info.input_rate; out.sampleRate = info.sample_rate;
        out.fft_size = info.fft_size; out.fft_floor = info.fft_floor; out.fft_ceil = info.fft_ceil;
        return out;
    }

private:
    static constexpr int kMaxFrameFloats = 4096;
    void pushEnables() { (void)errlog.ok(csdr_scopebank_set_enabled(sb_, scopeOn_ ? 1 : 0, spectrumOn_ ? 1 : 0), "csdr_scopebank_set_enabled"); }
    csdr_scopebank *sb_ = nullptr;
    int fftSize_ = 0;
    bool scopeOn_ = true, spectrumOn_ = true;
};
