// DemodDensity.h -- the persistence ("digital phosphor") display for any number of demodulators at once: for every pixel of a spectrum or scope
// tile, how often the trace passed through it, as tiles of one RGBA8 atlas with the geometry of DemodWaterfallBank::renderView and
// DemodTraceBank::render; own implementation -- the reference has the idea only as ScopePanel's 0.05-alpha background (src/panel/ScopePanel.cpp:88-89).
//
// The bank is a csdr_density (include/csdr_hip.h, "Density bank"): the hit grids live in HBM, a step is two device launches whatever the number of
// slots and frames, and the frames are read where the spectrum, view and scope banks left them.  There is NO host arithmetic here: what makes this
// display affordable is that the frames never leave the device, so a bank without a context does not exist and the constructor throws.  The
// rule itself is available without a device as csdr_design_density_cover.
#pragma once
#include <stdexcept>
#include <vector>

#include "HipPipeline.h"

class DemodDensityBank {
public:
    // csdr_density_item's fields
    struct Item { int slot; const float *points; int n; int frames; long long strideFloats; int layout; int kind; int isDev; unsigned keepQ16; unsigned weight; };
    struct View { int slot; unsigned full; };

    explicit DemodDensityBank(csdr_ctx *ctx) {
        if (!ctx) throw std::invalid_argument("DemodDensityBank needs a context: the hit grids live on the device");
        csdr_must(csdr_density_create(ctx, &db_), "csdr_density_create");
    }
    ~DemodDensityBank() { if (db_) csdr_density_destroy(db_); }
    DemodDensityBank(const DemodDensityBank &) = delete;
    DemodDensityBank &operator=(const DemodDensityBank &) = delete;
    csdr_density *handle() { return db_; }
    CsdrErrorLog errlog;

    bool setup(int width, int height, int maxSlots, int maxFrames, int maxPoints) {
        if (!errlog.ok(csdr_density_setup(db_, width, height, maxSlots, maxFrames, maxPoints), "csdr_density_setup")) return false;
        width_ = width; height_ = height;
        return true;
    }
    bool setPalette(const unsigned char *rgba /*[256][4]*/) { return errlog.ok(csdr_density_set_palette(db_, rgba), "csdr_density_set_palette"); }
    bool resetSlot(int slot) { return errlog.ok(csdr_density_reset_slot(db_, slot), "csdr_density_reset_slot"); }
    bool step(const std::vector<Item> &items) {
        std::vector<csdr_density_item> it(items.size());
        for (size_t k = 0; k < items.size(); ++k)
            it[k] = csdr_density_item{items[k].points, items[k].strideFloats, items[k].slot, items[k].n, items[k].frames, items[k].layout, items[k].kind,
                                      items[k].isDev, items[k].keepQ16, items[k].weight};
        return errlog.ok(csdr_density_step(db_, it.data(), (int)it.size()), "csdr_density_step");
    }
    bool stepSpectrum(int slot, csdr_spec *spec, int frame0, int nFrames, unsigned keepQ16, unsigned weight) {
        return errlog.ok(csdr_density_step_spec(db_, slot, spec, frame0, nFrames, keepQ16, weight), "csdr_density_step_spec");
    }
    bool stepSpectrumBank(csdr_specbank *sb, unsigned keepQ16, unsigned weight) {
        return errlog.ok(csdr_density_step_specbank(db_, sb, keepQ16, weight), "csdr_density_step_specbank");
    }
    bool peak(int slot, unsigned &out) {
        uint32_t v = 0;
        const bool ok = errlog.ok(csdr_density_peak(db_, slot, &v), "csdr_density_peak");
        out = v;
        return ok;
    }
    bool fetch(int slot, std::vector<uint32_t> &out) {
        out.assign((size_t)width_ * (size_t)height_, 0);
        return errlog.ok(csdr_density_fetch(db_, slot, out.data(), (int64_t)out.size()), "csdr_density_fetch");
    }
    // the views as tiles of ONE RGBA8 picture, atlasCols tiles to a tile row (csdr_hip.h, "Density bank", item 4); false: refused, nothing rendered
    bool render(const std::vector<View> &views, int atlasCols, std::vector<unsigned char> &out) {
        const int n = (int)views.size();
        const size_t rows = atlasCols > 0 ? (size_t)((n + atlasCols - 1) / atlasCols) : 0;
        std::vector<csdr_density_view> v(views.size());
        for (size_t k = 0; k < views.size(); ++k) v[k] = csdr_density_view{views[k].slot, views[k].full};
        out.assign(rows * (size_t)height_ * (size_t)(atlasCols > 0 ? atlasCols : 0) * (size_t)width_ * 4, 0);
        return errlog.ok(csdr_density_render(db_, v.data(), n, atlasCols, out.data(), (int64_t)out.size()), "csdr_density_render");
    }

private:
    csdr_density *db_ = nullptr;
    int width_ = 0, height_ = 0;
};
