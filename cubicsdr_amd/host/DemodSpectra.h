// DemodSpectra.h -- a spectrum per demodulator: N SpectrumVisualProcessors (full-span view) fed the demodulators' resampled IQ, with the setters'
// names of the reference's src/process/SpectrumVisualProcessor.h applied to all of them; own implementation.  The reference shows this picture for the
// ACTIVE demodulator only (CubicSDR.cpp:373-381); a station that demodulates hundreds of channels on one device wants it for each.
//
// With a context the bank is a csdr_specbank (include/csdr_hip.h, "Spectrum bank"): state and points stay in HBM, and process(bank) is ONE device
// call behind csdr_bank_execute -- every slot and every block of the execute in one launch, no host synchronisation.  Without a context
// (ctx == nullptr) the same arithmetic runs on the host, spelled out below as the reference spells it (file:line of SpectrumVisualProcessor.cpp) --
// for a build without a device and as a yardstick of the tests.  The two agree to the float32 transform's rounding, not bit for bit: the host's
// transform is a plain radix-2 one.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "HipPipeline.h"

class DemodSpectrumBank {
public:
    struct Item { int slot; const liquid_float_complex_t *data; int n; };      // one process() input of a slot; n == 0: no input at all

    explicit DemodSpectrumBank(csdr_ctx *ctx = nullptr) : ctx_(ctx) {
        if (ctx_) csdr_must(csdr_specbank_create(ctx_, &sb_), "csdr_specbank_create");
    }
    ~DemodSpectrumBank() { if (sb_) csdr_specbank_destroy(sb_); }
    DemodSpectrumBank(const DemodSpectrumBank &) = delete;
    DemodSpectrumBank &operator=(const DemodSpectrumBank &) = delete;
    bool onDevice() const { return sb_ != nullptr; }
    csdr_specbank *handle() { return sb_; }
    CsdrErrorLog errlog;

    // setup(fftSize_in) (:140-178) for every slot; false: the size or the counts are refused (csdr_hip.h, "Spectrum bank", item 1)
    bool setup(unsigned int fftSize_in, int maxSlots, int maxFrames) {
        if (sb_) {
            if (!errlog.ok(csdr_specbank_setup(sb_, (int)fftSize_in, maxSlots, maxFrames), "csdr_specbank_setup")) return false;
        } else {
            if (fftSize_in < 8 || (fftSize_in & (fftSize_in - 1)) || fftSize_in > 2048 || maxSlots < 1 || maxSlots > 4096 || maxFrames < 1)
                return errlog.ok(fftSize_in >= 8 && maxSlots >= 1 && maxSlots <= 4096 && maxFrames >= 1 ? CSDR_EUNSUPPORTED : CSDR_EINVAL, "DemodSpectrumBank::setup");
            slots_.assign((size_t)maxSlots, Slot());
            for (Slot &s : slots_) freshSlot(s, 2 * fftSize_in);
            tw_.resize(fftSize_in);                                                   // exp(-2 pi i k / Fi), k < Fi / 2
            for (unsigned int k = 0; k < fftSize_in; ++k) {
                const double a = -2.0 * M_PI * (double)k / (double)(2 * fftSize_in);
                tw_[k] = {(float)std::cos(a), (float)std::sin(a)};
            }
        }
        fftSize = fftSize_in; fftSizeInternal = 2 * fftSize_in;                       // SPECTRUM_VZM (.h:11)
        maxSlots_ = maxSlots; maxFrames_ = maxFrames;
        return true;
    }
    void setFFTAverageRate(float fftAverageRate) { fft_average_rate = fftAverageRate; if (sb_) (void)errlog.ok(csdr_specbank_set_average_rate(sb_, fftAverageRate), "csdr_specbank_set_average_rate"); }
    float getFFTAverageRate() const { return fft_average_rate; }
    void setScaleFactor(float sf) { scaleFactor = sf; if (sb_) (void)errlog.ok(csdr_specbank_set_scale_factor(sb_, sf), "csdr_specbank_set_scale_factor"); }
    float getScaleFactor() const { return scaleFactor; }
    void setPeakHold(bool peakHold_in) {                                             // :115-125, on every slot
        if (sb_) { (void)errlog.ok(csdr_specbank_set_peak_hold(sb_, peakHold_in ? 1 : 0), "csdr_specbank_set_peak_hold"); peakHold = csdr_specbank_get_peak_hold(sb_) != 0; return; }
        const bool again = peakHold && peakHold_in;
        for (Slot &s : slots_) s.peakReset = again ? 30 : 1;                         // PEAK_RESET_COUNT (.h:12)
        if (!again) peakHold = peakHold_in;
    }
    bool getPeakHold() const { return peakHold; }
    bool resetSlot(int slot) {
        if (sb_) return errlog.ok(csdr_specbank_reset_slot(sb_, slot), "csdr_specbank_reset_slot");
        if (slot < 0 || slot >= maxSlots_) return errlog.ok(CSDR_EINVAL, "DemodSpectrumBank::resetSlot");
        freshSlot(slots_[(size_t)slot], fftSizeInternal);
        return true;
    }

    // every block of the bank's last csdr_bank_execute, for every active slot: with a context ONE device call where the samples lie; without, the
    // host fetches each slot's resampled IQ (csdr_bank_fetch_iq, cut by csdr_block_result.n_iq) and runs the arithmetic below
    bool process(csdr_bank *bank, int bankSlots, int maxBlocks) {
        if (sb_) return errlog.ok(csdr_specbank_process_bank(sb_, bank), "csdr_specbank_process_bank");
        std::vector<std::vector<liquid_float_complex_t>> iq((size_t)bankSlots);
        std::vector<Item> items;
        std::vector<csdr_block_result> res((size_t)maxBlocks);
        for (int s = 0; s < bankSlots && s < maxSlots_; ++s) {
            int nb = 0, n = 0;
            if (!errlog.ok(csdr_bank_fetch_results(bank, s, res.data(), maxBlocks, &nb), "csdr_bank_fetch_results")) return false;
            long long total = 0;
            for (int b = 0; b < nb; ++b) total += res[(size_t)b].n_iq;
            if (total == 0) continue;
            iq[(size_t)s].resize((size_t)total);
            if (!errlog.ok(csdr_bank_fetch_iq(bank, s, &iq[(size_t)s][0].real, (int)total, &n), "csdr_bank_fetch_iq") || n != total) return false;
            long long at = 0;
            for (int b = 0; b < nb; ++b) { items.push_back(Item{s, iq[(size_t)s].data() + at, res[(size_t)b].n_iq}); at += res[(size_t)b].n_iq; }
        }
        return process(items);
    }
    // the items of one slot are its inputs in the order given; a call that would give a slot more than maxFrames frames is refused as a whole
    bool process(const std::vector<Item> &items) {
        if (sb_) {
            std::vector<csdr_specbank_item> it(items.size());
            for (size_t k = 0; k < items.size(); ++k) it[k] = csdr_specbank_item{items[k].slot, items[k].n, items[k].data ? &items[k].data->real : nullptr, 0, 0};
            return errlog.ok(csdr_specbank_process(sb_, it.data(), (int)it.size()), "csdr_specbank_process");
        }
        // the plan first (frame selection from the lengths alone, :387-421): a refused call changes nothing
        std::vector<int> frames((size_t)maxSlots_, 0);
        std::vector<unsigned int> lastSize((size_t)maxSlots_);
        for (int s = 0; s < maxSlots_; ++s) lastSize[(size_t)s] = slots_[(size_t)s].lastDataSize;
        for (const Item &it : items) {
            if (it.slot < 0 || it.slot >= maxSlots_ || it.n < 0 || (it.n > 0 && !it.data)) return errlog.ok(CSDR_EINVAL, "DemodSpectrumBank::process");
            if (it.n == 0) continue;
            unsigned int &ls = lastSize[(size_t)it.slot];
            if ((unsigned int)it.n < fftSizeInternal && ls + (unsigned int)it.n < fftSizeInternal) ls += std::max(fftSizeInternal - ls, (unsigned int)it.n);
            else if (++frames[(size_t)it.slot] > maxFrames_) return errlog.ok(CSDR_ERANGE, "DemodSpectrumBank::process");
        }
        for (Slot &s : slots_) s.out.clear();
        for (const Item &it : items) if (it.n > 0) processInput(slots_[(size_t)it.slot], it.data, (unsigned int)it.n);
        return true;
    }
    int frames(int slot) const {
        if (sb_) return csdr_specbank_frames(sb_, slot);
        return slot >= 0 && slot < maxSlots_ ? (int)slots_[(size_t)slot].out.size() : 0;
    }
    // SpectrumVisualData of a frame of the last process call (spectrum_hold_points empty when the frame carries none)
    bool fetch(int slot, int frame, SpectrumVisualData &out) {
        if (sb_) {
            out.spectrum_points.resize((size_t)fftSize * 2);
            out.spectrum_hold_points.resize((size_t)fftSize * 2);
            int nh = 0;
            if (!errlog.ok(csdr_specbank_fetch(sb_, slot, frame, out.spectrum_points.data(), (int)out.spectrum_points.size(), &out.fft_ceiling, &out.fft_floor), "csdr_specbank_fetch")) return false;
            if (!errlog.ok(csdr_specbank_fetch_hold(sb_, slot, frame, out.spectrum_hold_points.data(), (int)out.spectrum_hold_points.size(), &nh), "csdr_specbank_fetch_hold")) return false;
            out.spectrum_hold_points.resize((size_t)nh);
            return true;
        }
        if (slot < 0 || slot >= maxSlots_ || frame < 0 || frame >= (int)slots_[(size_t)slot].out.size()) return errlog.ok(CSDR_EINVAL, "DemodSpectrumBank::fetch");
        out = slots_[(size_t)slot].out[(size_t)frame];
        return true;
    }
    // a slot's lines of the last call into a waterfall panel of the same fft size: on the device from where they lie (csdr_specbank_device_points)
    bool stepInto(int slot, csdr_waterfall *wf) {
        if (!sb_) return errlog.ok(CSDR_ESTATE, "DemodSpectrumBank::stepInto needs a device bank");
        const float *dev = nullptr;
        int n = 0;
        if (!errlog.ok(csdr_specbank_device_points(sb_, slot, &dev, &n), "csdr_specbank_device_points")) return false;
        return n == 0 || errlog.ok(csdr_waterfall_step(wf, dev, 1, (int)fftSize, n, nullptr), "csdr_waterfall_step");
    }

private:
    struct Slot {                                                                     // the reference's members, per processor
        std::vector<liquid_float_complex_t> fftLastData;
        std::vector<double> fft_result_ma, fft_result_maa, fft_result_peak;
        double fft_ceil_ma = 100.0, fft_ceil_maa = 100.0, fft_floor_ma = 0.0, fft_floor_maa = 0.0;      // ctor :32-33
        double fft_ceil_peak = 0.0, fft_floor_peak = 0.0;
        unsigned int lastDataSize = 0;
        int peakReset = 0;
        std::vector<SpectrumVisualData> out;
    };
    void freshSlot(Slot &s, unsigned int n) {
        s = Slot();
        s.fftLastData.assign(n, liquid_float_complex_t{0.f, 0.f});
        s.fft_result_ma.assign(n, 0.0); s.fft_result_maa.assign(n, 0.0); s.fft_result_peak.assign(n, 0.0);
        s.peakReset = 1;                                                              // setPeakHold(the bank's setting), once
    }
    // forward transform of fftSizeInternal points, float32: bit reversal, then radix-2 stages
    void fft(std::vector<liquid_float_complex_t> &x) const {
        const unsigned int n = fftSizeInternal;
        for (unsigned int i = 1, j = 0; i < n; ++i) {
            unsigned int bit = n >> 1;
            for (; j & bit; bit >>= 1) j ^= bit;
            j ^= bit;
            if (i < j) std::swap(x[i], x[j]);
        }
        for (unsigned int len = 2; len <= n; len <<= 1) {
            const unsigned int step = n / len;
            for (unsigned int i = 0; i < n; i += len)
                for (unsigned int k = 0; k < len / 2; ++k) {
                    const liquid_float_complex_t w = tw_[k * step], a = x[i + k], b = x[i + k + len / 2];
                    const liquid_float_complex_t t = {b.real * w.real - b.imag * w.imag, b.real * w.imag + b.imag * w.real};
                    x[i + k] = {a.real + t.real, a.imag + t.imag};
                    x[i + k + len / 2] = {a.real - t.real, a.imag - t.imag};
                }
        }
    }
    void processInput(Slot &s, const liquid_float_complex_t *data, unsigned int num_written) {
        const unsigned int N = fftSizeInternal;
        const bool doPeak = peakHold && (s.peakReset == 0);                           // :247
        if (s.peakReset != 0) {                                                       // :264-273
            s.peakReset--;
            if (s.peakReset == 0) {
                for (unsigned int i = 0; i < N; i++) s.fft_result_peak[i] = s.fft_floor_maa;
                s.fft_ceil_peak = s.fft_floor_maa;
                s.fft_floor_peak = s.fft_ceil_maa;
            }
        }
        std::vector<liquid_float_complex_t> fftInput(N, liquid_float_complex_t{0.f, 0.f});
        if (num_written >= N) {                                                       // :401-404
            std::memcpy(fftInput.data(), data, N * sizeof(liquid_float_complex_t));
            s.fftLastData = fftInput;
        } else if (s.lastDataSize + num_written < N) {                                // priming :407-413
            unsigned int num_copy = N - s.lastDataSize;
            if (num_written > num_copy) num_copy = num_written;
            std::memcpy(fftInput.data(), data, num_written * sizeof(liquid_float_complex_t));       // (fftInData: the data, zero padded :391-393)
            std::memcpy(s.fftLastData.data(), fftInput.data(), num_copy * sizeof(liquid_float_complex_t));
            s.lastDataSize += num_copy;
            return;
        } else {                                                                      // :415-419
            const unsigned int num_last = N - num_written;
            std::memcpy(fftInput.data(), s.fftLastData.data() + (s.lastDataSize - num_last), num_last * sizeof(liquid_float_complex_t));
            std::memcpy(fftInput.data() + num_last, data, num_written * sizeof(liquid_float_complex_t));
            s.fftLastData = fftInput;
        }
        SpectrumVisualData output;
        output.spectrum_points.resize((size_t)fftSize * 2);
        if (doPeak) output.spectrum_hold_points.resize((size_t)fftSize * 2);
        float fft_ceil = 0, fft_floor = 1;
        fft(fftInput);                                                                // :439
        std::vector<float> fft_result(N);
        for (unsigned int i = 0, iMax = N / 2; i < iMax; i++) {                       // :441-452
            const float a = fftInput[i].real, b = fftInput[i].imag;
            volatile float aa = a * a, bb = b * b;
            const float c = std::sqrt(aa + bb);
            const float x = fftInput[N / 2 + i].real, y = fftInput[N / 2 + i].imag;
            volatile float xx = x * x, yy = y * y;
            const float z = std::sqrt(xx + yy);
            fft_result[i] = z;
            fft_result[N / 2 + i] = c;
        }
        for (unsigned int i = 0; i < N; i++) {                                        // :494-511
            if (s.fft_result_maa[i] != s.fft_result_maa[i]) s.fft_result_maa[i] = fft_result[i];
            s.fft_result_maa[i] += (s.fft_result_ma[i] - s.fft_result_maa[i]) * fft_average_rate;
            if (s.fft_result_ma[i] != s.fft_result_ma[i]) s.fft_result_ma[i] = fft_result[i];
            s.fft_result_ma[i] += (fft_result[i] - s.fft_result_ma[i]) * fft_average_rate;
            if (s.fft_result_maa[i] > fft_ceil || fft_ceil != fft_ceil) fft_ceil = (float)s.fft_result_maa[i];
            if (s.fft_result_maa[i] < fft_floor || fft_floor != fft_floor) fft_floor = (float)s.fft_result_maa[i];
            if (doPeak && s.fft_result_maa[i] > s.fft_result_peak[i]) s.fft_result_peak[i] = s.fft_result_maa[i];
        }
        if (s.fft_ceil_ma != s.fft_ceil_ma) s.fft_ceil_ma = fft_ceil;                 // :513-521
        s.fft_ceil_ma = s.fft_ceil_ma + (fft_ceil - s.fft_ceil_ma) * 0.05;
        if (s.fft_ceil_maa != s.fft_ceil_maa) s.fft_ceil_maa = fft_ceil;
        s.fft_ceil_maa = s.fft_ceil_maa + (s.fft_ceil_ma - s.fft_ceil_maa) * 0.05;
        if (s.fft_floor_ma != s.fft_floor_ma) s.fft_floor_ma = fft_floor;
        s.fft_floor_ma = s.fft_floor_ma + (fft_floor - s.fft_floor_ma) * 0.05;
        if (s.fft_floor_maa != s.fft_floor_maa) s.fft_floor_maa = fft_floor;
        s.fft_floor_maa = s.fft_floor_maa + (s.fft_floor_ma - s.fft_floor_maa) * 0.05;
        if (doPeak) {                                                                 // :523-530
            if (s.fft_ceil_maa > s.fft_ceil_peak) s.fft_ceil_peak = s.fft_ceil_maa;
            if (s.fft_floor_maa < s.fft_floor_peak) s.fft_floor_peak = s.fft_floor_maa;
        }
        const float sf = scaleFactor;
        const double point_ceil = doPeak ? s.fft_ceil_peak : s.fft_ceil_maa, point_floor = doPeak ? s.fft_floor_peak : s.fft_floor_maa;      // :539-540
        for (unsigned int x = 0, xMax = fftSize; x < xMax; x++) {                     // :542-576 at visualRatio 1: bins 2x and 2x + 1
            const double acc = (x == 0 ? s.fft_floor_maa : s.fft_result_maa[2 * x]) + s.fft_result_maa[2 * x + 1];
            output.spectrum_points[x * 2] = ((float)x / (float)xMax);
            output.spectrum_points[x * 2 + 1] = (float)(((std::log10((acc / 2.0) + 0.25 - (point_floor - 0.75)) / std::log10((point_ceil + 0.25) - (point_floor - 0.75)))) * sf);
            if (doPeak) {
                const double peak_acc = (x == 0 ? s.fft_floor_maa : s.fft_result_peak[2 * x]) + s.fft_result_peak[2 * x + 1];
                output.spectrum_hold_points[x * 2] = ((float)x / (float)xMax);
                output.spectrum_hold_points[x * 2 + 1] = (float)(((std::log10((peak_acc / 2.0) + 0.25 - (point_floor - 0.75)) / std::log10((point_ceil + 0.25) - (point_floor - 0.75)))) * sf);
            }
        }
        output.fft_ceiling = point_ceil / sf;                                         // :626-627
        output.fft_floor = point_floor;
        s.out.push_back(std::move(output));
    }

    csdr_ctx *ctx_;
    csdr_specbank *sb_ = nullptr;
    unsigned int fftSize = 0, fftSizeInternal = 0;
    int maxSlots_ = 0, maxFrames_ = 0;
    float fft_average_rate = 0.65f, scaleFactor = 1.0f;                               // :36
    bool peakHold = false;
    std::vector<Slot> slots_;
    std::vector<liquid_float_complex_t> tw_;
};
