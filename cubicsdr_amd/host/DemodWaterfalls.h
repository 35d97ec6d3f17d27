// DemodWaterfalls.h -- a waterfall per demodulator: N WaterfallPanels of one fft size and one number of lines, with the method names of the
// reference's src/panel/WaterfallPanel.h per slot; own implementation.  The reference draws this panel for the ACTIVE demodulator only
// (DEFAULT_DMOD_FFT_SIZE x DEFAULT_DEMOD_WATERFALL_LINES_NB); a station that demodulates hundreds of channels on one device wants a wall of them.
//
// With a context the bank is a csdr_wfbank (include/csdr_hip.h, "Waterfall bank"): lines, textures and pictures stay in HBM, every method is ONE
// device call -- whatever the number of slots it concerns -- and stepFrom() takes every slot's lines straight from a DemodSpectrumBank's points.
// Without a context (ctx == nullptr) the same statements run on the host: the bank then HOLDS ONE HOST WaterfallPanel PER SLOT
// (WaterfallPanel.h) and adds only what a panel does not have, the refusals and the atlas -- for a build without a device and as a yardstick of the
// tests; both give the same bytes.  Which of the two a bank is, is decided by its constructor and never changes.
#pragma once
#include <cstring>
#include <memory>
#include <vector>

#include "DemodSpectra.h"
#include "WaterfallPanel.h"

class DemodWaterfallBank {
public:
    // n_lines lines of n_floats floats for one slot (setPoints + step for each); points == nullptr or a wrong length repeats the slot's points
    struct Item { int slot; const float *points; int n_floats; int n_lines; };

    explicit DemodWaterfallBank(csdr_ctx *ctx = nullptr, int maxPending = 256) : ctx_(ctx), maxPending_(maxPending) {
        if (ctx_) csdr_must(csdr_wfbank_create(ctx_, &wb_), "csdr_wfbank_create");
    }
    ~DemodWaterfallBank() { if (wb_) csdr_wfbank_destroy(wb_); }
    DemodWaterfallBank(const DemodWaterfallBank &) = delete;
    DemodWaterfallBank &operator=(const DemodWaterfallBank &) = delete;
    bool onDevice() const { return wb_ != nullptr; }
    csdr_wfbank *handle() { return wb_; }
    CsdrErrorLog errlog;

    // setup(fft_size_in, num_waterfall_lines_in) (:13-24) on every slot; false: a size or a count is refused (csdr_hip.h, "Waterfall bank", item 1)
    bool setup(unsigned int fft_size_in, int num_waterfall_lines_in, int maxSlots) {
        if (wb_) {
            if (!errlog.ok(csdr_wfbank_setup(wb_, (int)fft_size_in, num_waterfall_lines_in, maxSlots, maxPending_), "csdr_wfbank_setup")) return false;
        } else {
            if (fft_size_in < 2 || fft_size_in > 4096 || num_waterfall_lines_in < 2 || num_waterfall_lines_in > 4096 || maxSlots < 1 || maxSlots > 4096 || maxPending_ < 1)
                return errlog.ok(CSDR_EINVAL, "DemodWaterfallBank::setup");
            panels_.resize((size_t)maxSlots);             // (a slot the bank had keeps its panel and so its points, :18-20)
            for (auto &p : panels_) {
                if (!p) p = freshPanel();
                p->setup(fft_size_in, num_waterfall_lines_in);
            }
        }
        fft_size = fft_size_in; waterfall_lines = num_waterfall_lines_in; maxSlots_ = maxSlots;
        staged_.assign((size_t)maxSlots, std::vector<float>());
        hasStaged_.assign((size_t)maxSlots, 0);
        return true;
    }
    // refreshTheme (:26-37) with Gradient::generate(256): one table for the bank
    bool setGradient(const std::vector<float> &rgbStops) {
        if (wb_) return errlog.ok(csdr_wfbank_set_gradient(wb_, rgbStops.data(), (int)(rgbStops.size() / 3)), "csdr_wfbank_set_gradient");
        float r[256], g[256], b[256];
        if (!errlog.ok(csdr_design_gradient(rgbStops.data(), (int)(rgbStops.size() / 3), 256, r, g, b), "csdr_design_gradient")) return false;
        stops_ = rgbStops;
        for (auto &p : panels_) if (p) p->setGradient(stops_);
        return true;
    }
    bool resetSlot(int slot) {
        if (wb_) return errlog.ok(csdr_wfbank_reset_slot(wb_, slot), "csdr_wfbank_reset_slot");
        if (slot < 0 || slot >= maxSlots_) return errlog.ok(CSDR_EINVAL, "DemodWaterfallBank::resetSlot");
        panels_[(size_t)slot] = freshPanel();
        panels_[(size_t)slot]->setup(fft_size, waterfall_lines);
        return true;
    }

    // setPoints (:39-49) of one slot: handed over by the slot's next step()
    void setPoints(int slot, std::vector<float> &points_in) {
        if (slot < 0 || slot >= maxSlots_) { (void)errlog.ok(CSDR_EINVAL, "DemodWaterfallBank::setPoints"); return; }
        staged_[(size_t)slot] = points_in;
        hasStaged_[(size_t)slot] = 1;
    }
    // step (:51-83) of one slot; false: refused
    bool step(int slot) {
        if (slot < 0 || slot >= maxSlots_) return errlog.ok(CSDR_EINVAL, "DemodWaterfallBank::step");
        const bool have = hasStaged_[(size_t)slot] != 0;
        hasStaged_[(size_t)slot] = 0;
        const std::vector<float> &pts = staged_[(size_t)slot];
        return step(std::vector<Item>{Item{slot, have ? pts.data() : nullptr, have ? (int)pts.size() : 0, 1}});
    }
    // the items of a slot are stepped in the order given; a call that would leave a slot with more than maxPending lines waiting, or that names a
    // slot the bank does not have, is refused as a whole and changes nothing
    bool step(const std::vector<Item> &items, std::vector<int> *taken = nullptr) {
        if (taken) taken->assign(items.size(), 0);
        if (wb_) {
            std::vector<csdr_wfbank_item> it(items.size());
            for (size_t k = 0; k < items.size(); ++k) it[k] = csdr_wfbank_item{items[k].slot, items[k].n_floats, items[k].points, 0, items[k].n_lines};
            return errlog.ok(csdr_wfbank_step(wb_, it.data(), (int)it.size(), taken ? taken->data() : nullptr), "csdr_wfbank_step");
        }
        std::vector<long long> add((size_t)maxSlots_, 0);
        for (const Item &it : items) {
            if (it.slot < 0 || it.slot >= maxSlots_ || it.n_lines < 0 || it.n_floats < 0) return errlog.ok(CSDR_EINVAL, "DemodWaterfallBank::step");
            WaterfallPanel &p = *panels_[(size_t)it.slot];
            if (p.getOffset(0) < 0) continue;             // no textures: the steps are dropped
            add[(size_t)it.slot] += it.n_lines;
            if (p.getLinesBuffered() + add[(size_t)it.slot] > maxPending_) return errlog.ok(CSDR_ERANGE, "DemodWaterfallBank::step");
        }
        std::vector<float> line;
        for (size_t k = 0; k < items.size(); ++k) {
            const Item &it = items[k];
            WaterfallPanel &p = *panels_[(size_t)it.slot];
            for (int l = 0; l < it.n_lines; ++l) {
                if (it.points) { line.assign(it.points + (size_t)l * it.n_floats, it.points + (size_t)(l + 1) * it.n_floats); p.setPoints(line); }
                const int before = p.getLinesBuffered();
                p.step();
                if (taken) (*taken)[k] += p.getLinesBuffered() - before;
            }
        }
        return true;
    }
    // every slot's frames of the spectrum bank's last process, HBM to HBM in one call (device banks only)
    bool stepFrom(DemodSpectrumBank &spectra, int *takenTotal = nullptr) {
        if (!wb_ || !spectra.onDevice()) return errlog.ok(CSDR_ESTATE, "DemodWaterfallBank::stepFrom needs a device bank and a device spectrum bank");
        return errlog.ok(csdr_wfbank_step_specbank(wb_, spectra.handle(), takenTotal), "csdr_wfbank_step_specbank");
    }
    void update() {                                                                  // :85-159 on every slot
        if (wb_) { (void)errlog.ok(csdr_wfbank_update(wb_), "csdr_wfbank_update"); return; }
        for (auto &p : panels_) p->update();
    }
    int getLinesBuffered(int slot) const {
        if (wb_) return csdr_wfbank_lines_buffered(wb_, slot);
        return slot >= 0 && slot < maxSlots_ ? panels_[(size_t)slot]->getLinesBuffered() : 0;
    }
    int getOffset(int slot, int half) const {
        if (wb_) return csdr_wfbank_offset(wb_, slot, half);
        return slot >= 0 && slot < maxSlots_ && (half == 0 || half == 1) ? panels_[(size_t)slot]->getOffset(half) : -1;
    }
    // one ring texture of one slot, waterfall_lines rows of fft_size / 2 bytes; false while the slot has no textures
    bool fetchIndex(int slot, int half, std::vector<unsigned char> &out) {
        if (wb_) {
            out.resize((size_t)(fft_size / 2) * (size_t)waterfall_lines);
            return errlog.ok(csdr_wfbank_fetch_index(wb_, slot, half, out.data(), (int64_t)out.size()), "csdr_wfbank_fetch_index");
        }
        if (slot < 0 || slot >= maxSlots_ || (half != 0 && half != 1)) return errlog.ok(CSDR_EINVAL, "DemodWaterfallBank::fetchIndex");
        return panels_[(size_t)slot]->fetchIndex(half, out);
    }
    // the listed slots' rings scaled to width x height tiles of ONE RGBA8 picture, atlasCols tiles to a tile row (csdr_hip.h, "Waterfall bank",
    // item 6): entry k at tile row k / atlasCols, tile column k % atlasCols; a slot without textures and the unused tiles are all-zero bytes
    bool renderView(const std::vector<int> &slots, int width, int height, int mode, int atlasCols, std::vector<unsigned char> &out) {
        const int n = (int)slots.size();
        if (wb_) {
            const size_t rows = atlasCols > 0 ? (size_t)((n + atlasCols - 1) / atlasCols) : 0;
            out.assign(rows * (size_t)std::max(height, 0) * (size_t)std::max(atlasCols, 0) * (size_t)std::max(width, 0) * 4, 0);
            return errlog.ok(csdr_wfbank_render(wb_, slots.data(), n, width, height, mode, atlasCols, out.data(), (int64_t)out.size()), "csdr_wfbank_render");
        }
        if (fft_size < 4 || width < 2 || width > 16384 || height < 1 || height > 16384 || (mode != CSDR_WF_VIEW_LINEAR && mode != CSDR_WF_VIEW_PEAK) ||
            n < 1 || atlasCols < 1 || atlasCols > n)
            return errlog.ok(CSDR_EINVAL, "DemodWaterfallBank::renderView");
        for (int s : slots) if (s < 0 || s >= maxSlots_) return errlog.ok(CSDR_EINVAL, "DemodWaterfallBank::renderView");
        const size_t W = (size_t)width, Hh = (size_t)height, picW = (size_t)atlasCols * W, rows = (size_t)((n + atlasCols - 1) / atlasCols);
        out.assign(rows * Hh * picW * 4, 0);
        std::vector<unsigned char> tile;
        for (int k = 0; k < n; ++k) {
            WaterfallPanel &p = *panels_[(size_t)slots[(size_t)k]];
            if (p.getOffset(0) < 0) continue;             // (:162-164: nothing is drawn)
            if (!p.renderView(width, height, mode, tile)) return errlog.ok(CSDR_EINVAL, "DemodWaterfallBank::renderView");
            for (size_t y = 0; y < Hh; ++y)
                std::memcpy(&out[((((size_t)k / (size_t)atlasCols) * Hh + y) * picW + ((size_t)k % (size_t)atlasCols) * W) * 4], &tile[y * W * 4], W * 4);
        }
        return true;
    }

private:
    std::unique_ptr<WaterfallPanel> freshPanel() {
        std::unique_ptr<WaterfallPanel> p(new WaterfallPanel(nullptr, maxPending_));
        if (!stops_.empty()) p->setGradient(stops_);
        return p;
    }
    csdr_ctx *ctx_;
    int maxPending_;
    csdr_wfbank *wb_ = nullptr;
    unsigned int fft_size = 0;
    int waterfall_lines = 0, maxSlots_ = 0;
    std::vector<std::vector<float>> staged_;              // setPoints(slot) until the slot's step()
    std::vector<char> hasStaged_;
    // host bank
    std::vector<std::unique_ptr<WaterfallPanel>> panels_;
    std::vector<float> stops_;
};
