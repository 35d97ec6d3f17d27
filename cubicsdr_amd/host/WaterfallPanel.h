// WaterfallPanel.h -- the waterfall's panel and the pacing rule that feeds it; API of the reference's src/panel/WaterfallPanel.h (setup, setPoints,
// step, update) and of WaterfallCanvas::processInputQueue (src/visual/WaterfallCanvas.cpp:89-126); own implementation.
//
// With a context the panel is a csdr_waterfall: lines are quantised, kept in the two ring textures and coloured in HBM (include/csdr_hip.h,
// "WaterfallPanel"), and stepFrom() takes a line straight from a SpectrumVisualProcessor's point buffer without a trip over the link.  Without a
// context (ctx == nullptr) the same arithmetic runs on the host, spelled out below as the reference spells it -- for a build without a device and
// as the yardstick of the tests; both give the same bytes.  renderView() is the picture scaled to a viewport (csdr_hip.h, "Waterfall viewport"):
// what drawPanelContents draws through GL, as bytes a headless consumer can use.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "HipPipeline.h"

class WaterfallPanel {
public:
    explicit WaterfallPanel(csdr_ctx *ctx = nullptr, int maxPending = 256) : ctx_(ctx), maxPending_(maxPending) {
        if (ctx_) csdr_must(csdr_waterfall_create(ctx_, &wf_), "csdr_waterfall_create");
        for (int i = 0; i < 256; ++i) { table_[4 * i] = table_[4 * i + 1] = table_[4 * i + 2] = (unsigned char)i; table_[4 * i + 3] = 255; }
    }
    ~WaterfallPanel() { if (wf_) csdr_waterfall_destroy(wf_); }
    WaterfallPanel(const WaterfallPanel &) = delete;
    WaterfallPanel &operator=(const WaterfallPanel &) = delete;
    bool onDevice() const { return wf_ != nullptr; }
    CsdrErrorLog errlog;

    void setup(unsigned int fft_size_in, int num_waterfall_lines_in) {               // :13-24
        waterfall_lines = num_waterfall_lines_in;
        fft_size = fft_size_in;
        if (wf_) { (void)errlog.ok(csdr_waterfall_setup(wf_, (int)fft_size, waterfall_lines, maxPending_), "csdr_waterfall_setup"); staged_ = false; return; }
        lines_buffered = 0;
        if (points.size() != fft_size) points.resize(fft_size);
        texInitialized = false;
        bufferInitialized = false;
    }
    // refreshTheme (:26-37) with Gradient::generate(256) (Gradient.cpp:37-85): colour stops r, g, b interleaved, the application's own data
    bool setGradient(const std::vector<float> &rgbStops) {
        const int n = (int)(rgbStops.size() / 3);
        if (wf_) return errlog.ok(csdr_waterfall_set_gradient(wf_, rgbStops.data(), n), "csdr_waterfall_set_gradient");
        float r[256], g[256], b[256];
        if (!errlog.ok(csdr_design_gradient(rgbStops.data(), n, 256, r, g, b), "csdr_design_gradient")) return false;
        auto u8 = [](float c) { volatile float p = c * 255.0f; const float q = p + 0.5f; return q >= 0.5f ? (unsigned char)q : (unsigned char)0; };
        for (int i = 0; i < 256; ++i) { table_[4 * i] = u8(r[i]); table_[4 * i + 1] = u8(g[i]); table_[4 * i + 2] = u8(b[i]); table_[4 * i + 3] = 255; }
        return true;
    }
    void setPoints(std::vector<float> &points_in) {                                  // :39-49
        if (wf_) { staged_points_ = points_in; staged_ = true; return; }              // handed over by the next step()
        if (points_in.size() == (size_t)fft_size * 2) {
            for (unsigned int i = 0; i < fft_size; i++) points[i] = points_in[i * 2 + 1];
        } else if (points_in.size() == fft_size) {
            points.assign(points_in.begin(), points_in.end());
        }   // any other length leaves the points alone (what WaterfallCanvas.cpp:106-109 does with a frame of the wrong size)
    }
    void step() {                                                                    // :51-83
        if (wf_) {
            const bool have = staged_;
            staged_ = false;
            (void)errlog.ok(csdr_waterfall_step(wf_, have ? staged_points_.data() : nullptr, 0, have ? (int)staged_points_.size() : 0, 1, nullptr), "csdr_waterfall_step");
            return;
        }
        const unsigned int half_fft_size = fft_size / 2;
        bufferInitialized = true;
        if (!texInitialized) return;
        if (!points.empty() && points.size() == fft_size) {
            for (int j = 0; j < 2; j++) {
                const size_t at = lineBuffer[j].size();
                lineBuffer[j].resize(at + half_fft_size);
                for (unsigned int i = 0; i < half_fft_size; i++) {
                    const float v = points[j * half_fft_size + i];
                    float wv = v < 0 ? 0 : (v > 0.99 ? 0.99 : v);
                    if (wv != wv) wv = 0;                                            // a NaN gives 0 (the library's definition, csdr_hip.h)
                    lineBuffer[j][at + i] = (unsigned char)std::floor(wv * 255.0);
                }
            }
            lines_buffered++;
        }
    }
    // the line of frame 0 of the processor's last input, HBM to HBM (device panels only; call it from the thread that runs the processor)
    bool stepFrom(SpectrumVisualProcessor &proc) {
        if (!wf_) return errlog.ok(CSDR_ESTATE, "WaterfallPanel::stepFrom needs a device panel");
        staged_ = false;
        return errlog.ok(csdr_waterfall_step_spec(wf_, proc.handle(), 0, 1, nullptr), "csdr_waterfall_step_spec");
    }
    // the lines of frames frame0 .. frame0 + nFrames - 1 of the processor's last input (SpectrumVisualProcessor::processLines makes several)
    bool stepFrom(SpectrumVisualProcessor &proc, int frame0, int nFrames) {
        if (!wf_) return errlog.ok(CSDR_ESTATE, "WaterfallPanel::stepFrom needs a device panel");
        staged_ = false;
        return errlog.ok(csdr_waterfall_step_spec(wf_, proc.handle(), frame0, nFrames, nullptr), "csdr_waterfall_step_spec");
    }
    void update() {                                                                  // :85-159
        if (wf_) { (void)errlog.ok(csdr_waterfall_update(wf_), "csdr_waterfall_update"); return; }
        const unsigned int half_fft_size = fft_size / 2;
        if (!bufferInitialized) return;
        if (!texInitialized) {
            for (int i = 0; i < 2; i++) { waterfall_ofs[i] = waterfall_lines - 1; waterfall[i].assign((size_t)half_fft_size * waterfall_lines, 0); }
            texInitialized = true;
        }
        std::vector<unsigned char> rLineBuffer[2];
        for (int j = 0; j < 2; j++) {
            rLineBuffer[j].resize(lineBuffer[j].size());
            for (int i = 0, iMax = lines_buffered; i < iMax; i++)
                std::memcpy(&rLineBuffer[j][(size_t)i * half_fft_size], &lineBuffer[j][(size_t)(iMax - 1 - i) * half_fft_size], half_fft_size);
        }
        unsigned int run_ofs = 0;
        while (lines_buffered) {
            int run_lines = lines_buffered;
            if (run_lines > waterfall_ofs[0]) run_lines = waterfall_ofs[0];
            for (int j = 0; j < 2; j++) {
                std::memcpy(&waterfall[j][(size_t)(waterfall_ofs[j] - run_lines) * half_fft_size], &rLineBuffer[j][run_ofs], (size_t)run_lines * half_fft_size);
                waterfall_ofs[j] -= run_lines;
                if (waterfall_ofs[j] == 0) waterfall_ofs[j] = waterfall_lines;
            }
            run_ofs += run_lines * half_fft_size;
            lines_buffered -= run_lines;
        }
        lineBuffer[0].clear(); lineBuffer[1].clear();
    }
    int getLinesBuffered() const { return wf_ ? csdr_waterfall_lines_buffered(wf_) : lines_buffered; }
    int getOffset(int half) const { return wf_ ? csdr_waterfall_offset(wf_, half) : (texInitialized ? waterfall_ofs[half] : -1); }
    // one ring texture, waterfall_lines rows of fft_size / 2 bytes
    bool fetchIndex(int half, std::vector<unsigned char> &out) {
        const size_t n = (size_t)(fft_size / 2) * waterfall_lines;
        if (wf_) { out.resize(n); return errlog.ok(csdr_waterfall_fetch_index(wf_, half, out.data(), (int64_t)n), "csdr_waterfall_fetch_index"); }
        if (!texInitialized) return false;
        out = waterfall[half];
        return true;
    }
    // the picture drawPanelContents shows, unscaled (:186-213): row r is ring row (ofs + firstRow + r) mod lines, half 0 then half 1, RGBA8
    bool fetchRGBA(int firstRow, int nRows, std::vector<unsigned char> &out) {
        const size_t half = fft_size / 2;
        if (wf_) {
            out.resize((size_t)nRows * 2 * half * 4);
            return errlog.ok(csdr_waterfall_fetch_rgba(wf_, firstRow, nRows, out.data(), (int64_t)out.size()), "csdr_waterfall_fetch_rgba");
        }
        if (!texInitialized || firstRow < 0 || nRows < 1 || firstRow + nRows > waterfall_lines) return false;
        out.resize((size_t)nRows * 2 * half * 4);
        for (int r = 0; r < nRows; ++r) {
            const size_t row = (size_t)((waterfall_ofs[0] + firstRow + r) % waterfall_lines);
            for (int j = 0; j < 2; ++j)
                for (size_t i = 0; i < half; ++i)
                    std::memcpy(&out[(((size_t)r * 2 + j) * half + i) * 4], &table_[4 * waterfall[j][row * half + i]], 4);
        }
        return true;
    }

    // the ring scaled to width x height pixels of RGBA8 (:161-219 into a viewport): mode CSDR_WF_VIEW_LINEAR is the reference's GL_LINEAR / GL_REPEAT
    // picture, CSDR_WF_VIEW_PEAK the maximum index over each pixel's footprint (csdr_hip.h, "Waterfall viewport", items 2-4).  The taps are the
    // library's host-only design functions in both cases.
    bool renderView(int width, int height, int mode, std::vector<unsigned char> &out) {
        const size_t W = width > 0 ? (size_t)width : 0, Hh = height > 0 ? (size_t)height : 0;
        if (wf_) {
            out.resize(W * Hh * 4);
            return errlog.ok(csdr_waterfall_render_view(wf_, width, height, mode, out.data(), (int64_t)out.size()), "csdr_waterfall_render_view");
        }
        if (!texInitialized) return false;
        std::vector<csdr_view_tap> ct(W), rt(Hh);
        if (!errlog.ok(csdr_design_view_columns((int)fft_size, width, mode, ct.data()), "csdr_design_view_columns")) return false;
        if (!errlog.ok(csdr_design_view_rows(waterfall_lines, height, mode, rt.data()), "csdr_design_view_rows")) return false;
        const size_t half = fft_size / 2;
        const int L = waterfall_lines, ofs = waterfall_ofs[0];
        out.resize(W * Hh * 4);
        for (size_t py = 0; py < Hh; ++py)
            for (size_t px = 0; px < W; ++px) {
                const std::vector<unsigned char> &tex = waterfall[ct[px].half];
                unsigned char *o = &out[(py * W + px) * 4];
                if (mode == CSDR_WF_VIEW_PEAK) {
                    unsigned char best = 0;
                    for (int r = rt[py].first; r < rt[py].first + rt[py].count; ++r) {
                        const unsigned char *row = &tex[(size_t)((ofs + r) % L) * half];
                        for (int i = ct[px].first; i < ct[px].first + ct[px].count; ++i) if (row[i] > best) best = row[i];
                    }
                    std::memcpy(o, &table_[4 * best], 4);
                    continue;
                }
                const size_t j0 = (size_t)((ofs + rt[py].first + L) % L), j1 = (j0 + 1) % (size_t)L, i0 = (size_t)ct[px].first;
                const unsigned char *c00 = &table_[4 * tex[j0 * half + i0]], *c10 = &table_[4 * tex[j0 * half + i0 + 1]];
                const unsigned char *c01 = &table_[4 * tex[j1 * half + i0]], *c11 = &table_[4 * tex[j1 * half + i0 + 1]];
                auto lerp = [](float a, float b, float w) { volatile float d = b - a; volatile float m = w * d; volatile float r = a + m; return (float)r; };      // (volatile: each step stored as a float)
                for (int ch = 0; ch < 3; ++ch) {
                    const float top = lerp((float)c00[ch], (float)c10[ch], ct[px].frac), bot = lerp((float)c01[ch], (float)c11[ch], ct[px].frac);
                    volatile float m = lerp(top, bot, rt[py].frac);
                    o[ch] = (unsigned char)(m + 0.5f);
                }
                o[3] = 255;
            }
        return true;
    }

private:
    csdr_ctx *ctx_;
    int maxPending_;
    csdr_waterfall *wf_ = nullptr;
    std::vector<float> staged_points_;
    bool staged_ = false;
    // host panel: the reference's members
    std::vector<float> points;
    std::vector<unsigned char> lineBuffer[2], waterfall[2];
    unsigned int fft_size = 0;
    int waterfall_lines = 0, waterfall_ofs[2] = {0, 0}, lines_buffered = 0;
    bool texInitialized = false, bufferInitialized = false;
    unsigned char table_[1024];
};

// WaterfallCanvas::processInputQueue (:89-126) as a function of the elapsed seconds (gTimer.lastUpdateSeconds()), so that it can be driven without a
// clock: lpsIndex accumulates the time, one line is due per 1 / linesPerSecond, every due line pops one SpectrumVisualData -- a frame of
// fft_size * 2 points sets the panel's points, any other is stepped with the previous ones, a null entry only uses up its turn -- and the loop stops
// at an empty queue.  Returns true when a line was stepped; the panel has then been updated (:120-124).
struct WaterfallFeed {
    double lpsIndex = 0.0;
    int linesPerSecond = DEFAULT_WATERFALL_LPS;
    long stepped = 0;

    bool processInputQueue(double lastUpdateSeconds, SpectrumVisualDataQueue &visualDataQueue, WaterfallPanel &waterfallPanel, unsigned int fft_size) {
        const double targetVis = 1.0 / (double)linesPerSecond;
        lpsIndex += lastUpdateSeconds;
        bool updated = false;
        if (linesPerSecond) {
            if (lpsIndex >= targetVis) {
                while (lpsIndex >= targetVis) {
                    SpectrumVisualDataPtr vData;
                    if (visualDataQueue.try_pop(vData)) {
                        if (vData) {
                            if (vData->spectrum_points.size() == (size_t)fft_size * 2) waterfallPanel.setPoints(vData->spectrum_points);
                            waterfallPanel.step();
                            ++stepped;
                            updated = true;
                        }
                        lpsIndex -= targetVis;
                    } else break;
                }
            }
        }
        if (updated) waterfallPanel.update();
        return updated;
    }
};
