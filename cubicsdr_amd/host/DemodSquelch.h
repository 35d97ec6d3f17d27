// DemodSquelch.h -- the signal level, floor, ceiling and squelch of every demodulator of a bank: what DemodulatorThread::run keeps per thread
// (reference src/demod/DemodulatorThread.cpp:142-238, :318-345), with the setter names of src/demod/DemodulatorThread.h per slot, and the squelch
// options of the reference's recorder (src/audio/AudioSinkFileThread.h:16-21); own implementation.
//
// The bank is a csdr_squelch (include/csdr_hip.h, "Squelch bank"): every slot's trackers and the items of every block stay in HBM, and process() is ONE
// device call over all blocks of the bank's last execute -- the level sums are read where the demodulators left them.  The flags it leaves gate the
// mixer feed (AudioMixer::takeBankAudioSquelched, host/Adapters.h) and the recorder (record()).  As DemodScopes.h, the mirror has no host arithmetic:
// without a context the constructor throws.  host/DemodLevel.h remains the one-block, one-slot statement that HipPipeline steps.
#pragma once
#include <vector>

#include "HipPipeline.h"

class DemodSquelchBank {
public:
    enum SquelchOption { SQUELCH_RECORD_SILENCE = 0, SQUELCH_SKIP_SILENCE = 1, SQUELCH_RECORD_ALWAYS = 2 };      // AudioSinkFileThread.h:16-21

    DemodSquelchBank(csdr_ctx *ctx, int maxSlots, int maxBlocks) : set_((size_t)(maxSlots > 0 ? maxSlots : 0)), maxBlocks_(maxBlocks) {
        csdr_must(csdr_squelch_create(ctx, maxSlots, maxBlocks, &sq_), "csdr_squelch_create");
    }
    ~DemodSquelchBank() { if (sq_) csdr_squelch_destroy(sq_); }
    DemodSquelchBank(const DemodSquelchBank &) = delete;
    DemodSquelchBank &operator=(const DemodSquelchBank &) = delete;
    csdr_squelch *handle() { return sq_; }
    CsdrErrorLog errlog;

    // the settings take effect at the next process() and are constant within it (the reference reads its atomics once per block)
    bool setSquelchEnabled(int slot, bool on) { return known(slot) && push(slot, [&](Settings &s) { s.enabled = on; }); }      // :384-390
    bool setSquelchLevel(int slot, float dB) { return known(slot) && push(slot, [&](Settings &s) { s.level = dB; s.enabled = true; }); }      // :392-397 switches it on
    bool setMuted(int slot, bool muted) { return known(slot) && push(slot, [&](Settings &s) { s.muted = muted; }); }            // :339-345
    bool setSquelchOption(int slot, int option) { return known(slot) && push(slot, [&](Settings &s) { s.option = option; }); }  // AudioSinkFileThread.cpp:19-25
    bool isSquelchEnabled(int slot) const { return slot >= 0 && slot < (int)set_.size() && set_[(size_t)slot].enabled; }
    float getSquelchLevel(int slot) const { return slot >= 0 && slot < (int)set_.size() ? set_[(size_t)slot].level : 0.0f; }
    bool isMuted(int slot) const { return slot >= 0 && slot < (int)set_.size() && set_[(size_t)slot].muted; }
    bool resetSlot(int slot) { return errlog.ok(csdr_squelch_reset_slot(sq_, slot), "csdr_squelch_reset_slot"); }              // the constructor's values (:20-27)

    // every block of the bank's last execute, HBM to HBM in one call
    bool process(csdr_bank *bank) { return errlog.ok(csdr_squelch_process_bank(sq_, bank), "csdr_squelch_process_bank"); }
    int blocks(int slot) const { return csdr_squelch_blocks(sq_, slot); }
    // the meters: getSignalLevel / getSignalFloor / getSignalCeil (:376-382), the state after the last process
    bool meters(int slot, float &signalLevel, float &signalFloor, float &signalCeil, bool &squelchBreak) {
        int brk = 0;
        if (!errlog.ok(csdr_squelch_get_state(sq_, slot, &signalLevel, &signalFloor, &signalCeil, &brk), "csdr_squelch_get_state")) return false;
        squelchBreak = brk != 0;
        return true;
    }
    // the slot's items of the last process (empty: nothing was stepped, or the slot is unknown -- logged)
    std::vector<csdr_squelch_item> items(int slot) {
        std::vector<csdr_squelch_item> out((size_t)(maxBlocks_ > 0 ? maxBlocks_ : 0));
        int n = 0;
        if (!errlog.ok(csdr_squelch_fetch(sq_, slot, out.data(), (int)out.size(), &n), "csdr_squelch_fetch")) n = 0;
        out.resize((size_t)n);
        return out;
    }
    // the recorder: every stepped slot's 16-bit PCM of the last process by its squelch option, packed in slot order; slot s owns
    // pcm[offsets[s] .. offsets[s + 1])
    bool record(std::vector<int16_t> &pcm, std::vector<int64_t> &offsets, size_t capSamples = (size_t)1 << 24) {
        pcm.resize(capSamples);
        offsets.assign(set_.size() + 1, 0);
        if (!errlog.ok(csdr_squelch_record(sq_, pcm.data(), (int64_t)pcm.size(), offsets.data()), "csdr_squelch_record")) { pcm.clear(); return false; }
        pcm.resize((size_t)offsets.back());
        return true;
    }

private:
    struct Settings { bool enabled = false, muted = false; float level = 0.0f; int option = SQUELCH_RECORD_SILENCE; };
    bool known(int slot) { return errlog.ok(slot >= 0 && slot < (int)set_.size() ? CSDR_OK : CSDR_EINVAL, "DemodSquelchBank: slot"); }
    template <typename F> bool push(int slot, F change) {
        Settings s = set_[(size_t)slot];
        change(s);
        if (!errlog.ok(csdr_squelch_set_slot(sq_, slot, s.enabled ? 1 : 0, s.level, s.muted ? 1 : 0, s.option), "csdr_squelch_set_slot")) return false;
        set_[(size_t)slot] = s;
        return true;
    }
    csdr_squelch *sq_ = nullptr;
    std::vector<Settings> set_;
    int maxBlocks_ = 0;
};
