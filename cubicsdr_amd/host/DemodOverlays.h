// DemodOverlays.h -- what the reference draws over a spectrum to say what it shows, for any number of tiles at once: the dB grid
// (src/panel/SpectrumPanel.cpp:117-147), the frequency ticks with their MHz labels and the two dB labels (:171-303) and a marker and a label per
// demodulator (src/visual/PrimaryGLContext.cpp:65-199), as ordered primitive lists composited onto the tiles of one RGBA8 atlas with the geometry of
// DemodTraceBank::render and DemodWaterfallBank::renderView; own implementation.
//
// With a context the bank is a csdr_overlay (include/csdr_hip.h, "Overlay bank"): a compose is ONE device call, whatever the number of tiles, and
// takes its base picture where a trace or waterfall bank left it in HBM.  Without a context (ctx == nullptr) the same picture is painted on the
// host by the header's rule, restated here; for a build without a device and as a yardstick of the tests; both give the same bytes.  Which of the
// two a bank is, is decided by its constructor and never changes.  The lists come from the library's planners (csdr_design_freq_scale, _db_grid,
// _db_labels, _demod_marker, _text), which need no device; text() below wraps the last.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "HipPipeline.h"

class DemodOverlayBank {
public:
    explicit DemodOverlayBank(csdr_ctx *ctx = nullptr) : ctx_(ctx) {
        if (ctx_) csdr_must(csdr_overlay_create(ctx_, &ov_), "csdr_overlay_create");
    }
    ~DemodOverlayBank() { if (ov_) csdr_overlay_destroy(ov_); }
    DemodOverlayBank(const DemodOverlayBank &) = delete;
    DemodOverlayBank &operator=(const DemodOverlayBank &) = delete;
    bool onDevice() const { return ov_ != nullptr; }
    csdr_overlay *handle() { return ov_; }
    CsdrErrorLog errlog;

    bool setup(int maxTiles, int maxPrims) {
        if (ov_) { if (!errlog.ok(csdr_overlay_setup(ov_, maxTiles, maxPrims), "csdr_overlay_setup")) return false; }
        else if (maxTiles < 1 || maxTiles > (1 << 20) || maxPrims < 1 || maxPrims > (1 << 22)) return errlog.ok(CSDR_EINVAL, "DemodOverlayBank::setup");
        maxTiles_ = maxTiles; maxPrims_ = maxPrims;
        return true;
    }
    // an 8-bit coverage plane, caller data; a8 == nullptr removes it
    bool setFont(const unsigned char *a8, int fontW, int fontH) {
        if (ov_) return errlog.ok(csdr_overlay_set_font(ov_, a8, fontW, fontH), "csdr_overlay_set_font");
        if (a8 && (fontW < 1 || fontW > 16384 || fontH < 1 || fontH > 16384)) return errlog.ok(CSDR_EINVAL, "DemodOverlayBank::setFont");
        font_.assign(a8 ? a8 : nullptr, a8 ? a8 + (size_t)fontW * (size_t)fontH : nullptr);
        fontW_ = a8 ? fontW : 0; fontH_ = a8 ? fontH : 0;
        return true;
    }
    // one string as masked primitives appended to `prims` (csdr_design_text)
    bool text(const std::vector<csdr_glyph> &glyphs, int lineHeight, const std::string &s, int x, int y, int halign, int valign, const unsigned char rgba[4], int mode,
              std::vector<csdr_overlay_prim> &prims) {
        const size_t at = prims.size();
        prims.resize(at + s.size());
        int n = 0;
        const bool ok = errlog.ok(csdr_design_text(glyphs.data(), (int)glyphs.size(), lineHeight, s.c_str(), x, y, halign, valign, rgba, mode, prims.data() + at, (int)s.size(), &n),
                                  "csdr_design_text");
        prims.resize(at + (ok ? (size_t)n : 0));
        return ok;
    }
    // tile k's list is prims[tiles[k].first .. + count) over tile k of `base` (host memory; nullptr: zero bytes; a device bank also takes device
    // memory with baseIsDev); the tiles of ONE RGBA8 picture, atlasCols to a tile row ("Overlay bank", items 1 - 4); false: refused, nothing composed
    bool compose(const unsigned char *base, bool baseIsDev, const std::vector<csdr_overlay_tile> &tiles, const std::vector<csdr_overlay_prim> &prims, int width, int height,
                 int atlasCols, std::vector<unsigned char> &out) {
        const int n = (int)tiles.size();
        const size_t rows = atlasCols > 0 ? (size_t)((n + atlasCols - 1) / atlasCols) : 0;
        const size_t bytes = rows * (size_t)std::max(height, 0) * (size_t)std::max(atlasCols, 0) * (size_t)std::max(width, 0) * 4;
        if (ov_) {
            out.assign(bytes, 0);
            return errlog.ok(csdr_overlay_compose(ov_, base, baseIsDev ? 1 : 0, tiles.data(), n, prims.data(), (int)prims.size(), width, height, atlasCols, out.data(),
                                                  (int64_t)out.size()), "csdr_overlay_compose");
        }
        if (maxTiles_ == 0) return errlog.ok(CSDR_ESTATE, "DemodOverlayBank::compose before setup");
        if (width < 1 || width > 16384 || height < 1 || height > 16384 || n < 1 || atlasCols < 1 || atlasCols > n || baseIsDev) return errlog.ok(CSDR_EINVAL, "DemodOverlayBank::compose");
        if (n > maxTiles_ || (long long)prims.size() > maxPrims_) return errlog.ok(CSDR_ERANGE, "DemodOverlayBank::compose");
        for (const csdr_overlay_tile &t : tiles)
            if (t.first < 0 || t.count < 0 || (long long)t.first + t.count > (long long)prims.size()) return errlog.ok(CSDR_EINVAL, "DemodOverlayBank::compose: run");
        for (const csdr_overlay_prim &q : prims) {
            bool bad = q.mode < CSDR_OVL_OVER || q.mode > CSDR_OVL_COPY || q.w < 0 || q.h < 0 || q.x < -(1 << 20) || q.x > (1 << 20) || q.y < -(1 << 20) || q.y > (1 << 20);
            if (!bad && q.mask_x >= 0) bad = fontW_ == 0 || q.mask_y < 0 || (long long)q.mask_x + q.w > fontW_ || (long long)q.mask_y + q.h > fontH_;
            if (bad) return errlog.ok(CSDR_EINVAL, "DemodOverlayBank::compose: primitive");
        }
        out.assign(bytes, 0);
        const size_t W = (size_t)width, picW = (size_t)atlasCols * W;
        for (int k = 0; k < n; ++k)
            for (int py = 0; py < height; ++py) {
                const size_t row = ((((size_t)k / (size_t)atlasCols) * (size_t)height + (size_t)py) * picW + ((size_t)k % (size_t)atlasCols) * W) * 4;
                if (base) std::memcpy(&out[row], base + row, W * 4);
                for (int i = tiles[(size_t)k].first; i < tiles[(size_t)k].first + tiles[(size_t)k].count; ++i) {
                    const csdr_overlay_prim &q = prims[(size_t)i];
                    if (py < q.y || (long long)py >= (long long)q.y + q.h) continue;
                    const int x0 = std::max(q.x, 0), x1 = (int)std::min<long long>((long long)q.x + q.w, width);
                    for (int px = x0; px < x1; ++px) paint(&out[row + (size_t)px * 4], q, px, py);
                }
            }
        return true;
    }

private:
    // item 4 of "Overlay bank": one pixel under one primitive that covers it
    void paint(unsigned char *d, const csdr_overlay_prim &q, int px, int py) const {
        unsigned a = q.rgba[3];
        if (q.mask_x >= 0) a = (a * font_[(size_t)(q.mask_y + (py - q.y)) * (size_t)fontW_ + (size_t)(q.mask_x + (px - q.x))] + 127u) / 255u;
        if (q.mode == CSDR_OVL_COPY) { d[0] = q.rgba[0]; d[1] = q.rgba[1]; d[2] = q.rgba[2]; d[3] = (unsigned char)a; return; }
        for (int ch = 0; ch < 4; ++ch) {
            const unsigned s = ch < 3 ? q.rgba[ch] : 255u;
            if (q.mode == CSDR_OVL_OVER) d[ch] = (unsigned char)((s * a + d[ch] * (255u - a) + 127u) / 255u);
            else d[ch] = (unsigned char)std::min(255u, d[ch] + (s * a + 127u) / 255u);
        }
    }
    csdr_ctx *ctx_;
    csdr_overlay *ov_ = nullptr;
    int maxTiles_ = 0, maxPrims_ = 0;
    std::vector<unsigned char> font_;
    int fontW_ = 0, fontH_ = 0;
};
