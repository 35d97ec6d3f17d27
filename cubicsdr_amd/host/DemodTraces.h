// DemodTraces.h -- the lines the reference draws above and beside a waterfall, for any number of demodulators at once: the spectrum trace with its
// peak-hold trace (src/panel/SpectrumPanel.cpp:117-160) and the scope trace in its three modes (src/panel/ScopePanel.cpp:30-112), as tiles of one
// RGBA8 atlas with the geometry of DemodWaterfallBank::renderView; own implementation.
//
// With a context the bank is a csdr_tracebank (include/csdr_hip.h, "Trace bank"): a render is ONE device call, whatever the number of items, and
// reads device points where the spectrum, view and scope banks left them.  Without a context (ctx == nullptr) the same picture is painted on the
// host: the lit intervals come from csdr_design_trace_envelope -- the library's one statement of the rule, which needs no device -- and this file
// adds the paint order, the XY points and the atlas; for a build without a device and as a yardstick of the tests; both give the same bytes.
// Which of the two a bank is, is decided by its constructor and never changes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "HipPipeline.h"

class DemodTraceBank {
public:
    // one tile: csdr_trace_item's fields; a host bank takes host points only
    struct Item { int kind; const float *points; const float *hold; int n; int layout; int isDev; };
    struct Colors { unsigned char bg[4] = {0, 0, 0, 255}, line[3] = {255, 255, 255}, hold[3] = {0, 255, 0}, axisMajor[3] = {255, 255, 255}, axisMinor[3] = {89, 89, 89}; };

    explicit DemodTraceBank(csdr_ctx *ctx = nullptr) : ctx_(ctx) {
        if (ctx_) csdr_must(csdr_tracebank_create(ctx_, &tb_), "csdr_tracebank_create");
    }
    ~DemodTraceBank() { if (tb_) csdr_tracebank_destroy(tb_); }
    DemodTraceBank(const DemodTraceBank &) = delete;
    DemodTraceBank &operator=(const DemodTraceBank &) = delete;
    bool onDevice() const { return tb_ != nullptr; }
    csdr_tracebank *handle() { return tb_; }
    CsdrErrorLog errlog;

    bool setup(int maxItems, int maxPoints) {
        if (tb_) { if (!errlog.ok(csdr_tracebank_setup(tb_, maxItems, maxPoints), "csdr_tracebank_setup")) return false; }
        else if (maxItems < 1 || maxItems > (1 << 20) || maxPoints < 1 || maxPoints > (1 << 21)) return errlog.ok(CSDR_EINVAL, "DemodTraceBank::setup");
        maxItems_ = maxItems; maxPoints_ = maxPoints;
        return true;
    }
    void setColors(const Colors &c) {
        colors_ = c;
        if (tb_) (void)errlog.ok(csdr_tracebank_set_colors(tb_, c.bg, c.line, c.hold, c.axisMajor, c.axisMinor), "csdr_tracebank_set_colors");
    }
    // the items as tiles of ONE RGBA8 picture, atlasCols tiles to a tile row (csdr_hip.h, "Trace bank", item 6); false: refused, nothing rendered
    bool render(const std::vector<Item> &items, int width, int height, int atlasCols, std::vector<unsigned char> &out) {
        const int n = (int)items.size();
        const size_t rows = atlasCols > 0 ? (size_t)((n + atlasCols - 1) / atlasCols) : 0;
        const size_t bytes = rows * (size_t)std::max(height, 0) * (size_t)std::max(atlasCols, 0) * (size_t)std::max(width, 0) * 4;
        if (tb_) {
            std::vector<csdr_trace_item> it(items.size());
            for (size_t k = 0; k < items.size(); ++k) it[k] = csdr_trace_item{items[k].points, items[k].hold, items[k].n, items[k].layout, items[k].kind, items[k].isDev};
            out.assign(bytes, 0);
            return errlog.ok(csdr_tracebank_render(tb_, it.data(), n, width, height, atlasCols, out.data(), (int64_t)out.size()), "csdr_tracebank_render");
        }
        if (maxItems_ == 0) return errlog.ok(CSDR_ESTATE, "DemodTraceBank::render before setup");
        if (width < 2 || width > 16384 || height < 1 || height > 16384 || n < 1 || n > maxItems_ || atlasCols < 1 || atlasCols > n)
            return errlog.ok(CSDR_EINVAL, "DemodTraceBank::render");
        for (const Item &it : items) {
            if (it.kind < CSDR_TRACE_SPECTRUM || it.kind > CSDR_TRACE_SCOPE_XY || (it.layout != 0 && it.layout != 1) || it.n < 0 || it.isDev != 0 ||
                (it.kind == CSDR_TRACE_SCOPE_2Y && height < 2))
                return errlog.ok(CSDR_EINVAL, "DemodTraceBank::render");
            if (it.n > maxPoints_) return errlog.ok(CSDR_ERANGE, "DemodTraceBank::render");
        }
        out.assign(bytes, 0);
        const size_t W = (size_t)width, picW = (size_t)atlasCols * W;
        std::vector<unsigned char> tile;
        for (int k = 0; k < n; ++k) {
            if (items[(size_t)k].n == 0 || !items[(size_t)k].points) continue;
            if (!paint(items[(size_t)k], width, height, tile)) return false;
            for (size_t y = 0; y < (size_t)height; ++y)
                std::memcpy(&out[((((size_t)k / (size_t)atlasCols) * (size_t)height + y) * picW + ((size_t)k % (size_t)atlasCols) * W) * 4], &tile[y * W * 4], W * 4);
        }
        return true;
    }

private:
    // item 1 of "Trace bank": the one float step
    static int quant(float y, float y0, float s, int N) {
        const float u = (y - y0) * s;
        if (!(u > 0.0f)) return 0;
        if (u >= 1.0f) return N - 1;
        return std::min(std::max((int)std::floor(u * (float)N), 0), N - 1);
    }
    static void put(unsigned char *px, const unsigned char *rgb) { px[0] = rgb[0]; px[1] = rgb[1]; px[2] = rgb[2]; }
    bool paint(const Item &it, int W, int H, std::vector<unsigned char> &t) {
        t.resize((size_t)W * (size_t)H * 4);
        for (size_t p = 0; p < (size_t)W * (size_t)H; ++p) std::memcpy(&t[4 * p], colors_.bg, 4);
        auto row = [&](int r, const unsigned char *rgb) { for (int c = 0; c < W; ++c) put(&t[((size_t)r * W + c) * 4], rgb); };
        if (it.kind == CSDR_TRACE_SCOPE_XY) {
            std::vector<int> hits((size_t)W * (size_t)H, 0);
            for (int k = 0; k < it.n / 2; ++k)
                ++hits[(size_t)(H - 1 - quant(it.points[2 * k + 1], -1.0f, 0.5f, H)) * W + quant(it.points[2 * k], -1.0f, 0.5f, W)];
            for (size_t p = 0; p < hits.size(); ++p)
                for (int ch = 0; ch < 3; ++ch) t[4 * p + ch] = (unsigned char)std::min<long long>(255, colors_.bg[ch] + (long long)hits[p] * colors_.line[ch]);
            return true;
        }
        if (it.kind == CSDR_TRACE_SCOPE_Y) row(H - 1 - quant(0.0f, -1.0f, 0.5f, H), colors_.axisMinor);
        if (it.kind == CSDR_TRACE_SCOPE_2Y) {
            const int hu = H / 2, hl = H - hu;
            row(hu - 1 - quant(0.0f, -1.0f, 0.5f, hu), colors_.axisMinor);
            row(hu + hl - 1 - quant(0.0f, -1.0f, 0.5f, hl), colors_.axisMinor);
            row(hu, colors_.axisMajor);
        }
        std::vector<int32_t> lo(2 * (size_t)W), hi(2 * (size_t)W);
        if (!errlog.ok(csdr_design_trace_envelope(it.points, it.kind == CSDR_TRACE_SPECTRUM ? it.hold : nullptr, it.n, it.layout, it.kind, W, H, lo.data(), hi.data()),
                       "csdr_design_trace_envelope")) return false;
        for (int which = 0; which < 2; ++which)
            for (int c = 0; c < W; ++c)
                for (int r = lo[(size_t)which * W + c]; r >= 0 && r <= hi[(size_t)which * W + c]; ++r) {
                    unsigned char *px = &t[((size_t)r * W + c) * 4];
                    if (which && it.kind == CSDR_TRACE_SPECTRUM) for (int ch = 0; ch < 3; ++ch) px[ch] = (unsigned char)((px[ch] + colors_.hold[ch] + 1) >> 1);
                    else put(px, colors_.line);
                }
        return true;
    }
    csdr_ctx *ctx_;
    csdr_tracebank *tb_ = nullptr;
    int maxItems_ = 0, maxPoints_ = 0;
    Colors colors_;
};
