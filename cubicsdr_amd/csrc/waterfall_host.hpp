// waterfall_host.hpp -- the host-side rules of WaterfallPanel (src/panel/WaterfallPanel.cpp) that csdr_waterfall.hip (one panel) and csdr_wfbank.hip
// (N panels per launch) both follow, stated once: the update plan, the cache of the viewport's tap tables, and the small pieces around them.
// Internal to those two units; the device-side counterpart is kernels_waterfall.hpp.
#pragma once
#include <vector>

#include "csdr_objects.hpp"

namespace csdr {

// WaterfallPanel::update's loop (:139-158) literally: runs of min(lines_buffered, waterfall_ofs[0]) rows at [ofs - run, ofs), an offset that reaches 0
// becomes waterfall_lines (both offsets move together: they start equal).  Only the first and the last run can be shorter than the ring; every run
// between them rewrites all of it.  So whatever came before the run in front of the last one is overwritten: the last two runs decide every row
// that changes, the later one where they overlap -- and only those two are kept, in the order the reference writes them (run[1] last).
struct WfUpdatePlan {
    WfRun run[2];
    int n_runs;                              // 1 or 2 (n_pending >= 1)
    int ofs;                                 // waterfall_ofs after the update
    int rows() const { return run[0].n + (n_runs > 1 ? run[1].n : 0); }
};
inline WfUpdatePlan wf_plan_update(int ofs, int lines, int n_pending) {
    WfUpdatePlan p{};
    int run_ofs = 0, left = n_pending;
    while (left) {
        const int run_lines = left < ofs ? left : ofs;
        p.run[0] = p.run[1];
        p.run[1] = WfRun{run_ofs, ofs - run_lines, run_lines};
        ++p.n_runs;
        ofs -= run_lines;
        if (ofs == 0) ofs = lines;
        run_ofs += run_lines;
        left -= run_lines;
    }
    if (p.n_runs == 1) { p.run[0] = p.run[1]; p.run[1] = WfRun{0, 0, 0}; }
    if (p.n_runs > 2) p.n_runs = 2;
    p.ofs = ofs;
    return p;
}

// The tap tables of (width, height, mode) on the device, [width] columns then [height] rows.  They depend on fft_size and lines (a setup forgets
// them) and not on the offset, so they are rebuilt only when one of the three changes.  on_design(taps) sees freshly designed tables on the host
// before anything of the cache is touched (the single panel derives its PEAK tiling there); if it refuses, the cache stays as it was.  Once it
// has accepted them the cache holds nothing until the upload is enqueued, so what on_design derived is never paired with older tables.
struct WfTapCache {
    DevBuf<csdr_view_tap> dev;
    std::vector<csdr_view_tap> host;         // (the upload's source: stays until the next rebuild)
    int w = 0, h = 0, mode = -1;             // what `dev` was designed for; mode -1: nothing
    void forget() { mode = -1; }
    template <typename OnDesign>
    int ensure(hipStream_t st, int fft_size, int lines, int width, int height, int mode_in, OnDesign &&on_design) {
        if (mode == mode_in && w == width && h == height) return CSDR_OK;
        std::vector<csdr_view_tap> t((size_t)width + (size_t)height);
        if (int rc = csdr_design_view_columns(fft_size, width, mode_in, t.data())) return rc;
        if (int rc = csdr_design_view_rows(lines, height, mode_in, t.data() + width)) return rc;
        if (int rc = on_design(t.data())) return rc;
        mode = -1;
        CSDR_HIP_TRY(hipStreamSynchronize(st));          // a kernel or an upload may still read what is replaced
        if (int rc = dev.reserve(t.size())) return rc;
        host.swap(t);
        CSDR_HIP_TRY(hipMemcpyAsync(dev.p, host.data(), host.size() * sizeof(csdr_view_tap), hipMemcpyHostToDevice, st));
        w = width; h = height; mode = mode_in;
        return CSDR_OK;
    }
    int ensure(hipStream_t st, int fft_size, int lines, int width, int height, int mode_in) {
        return ensure(st, fft_size, lines, width, height, mode_in, [](const csdr_view_tap *) { return CSDR_OK; });
    }
};

// what a viewport may be (csdr_hip.h, "Waterfall viewport")
inline int wf_check_view(int fft_size, int width, int height, int mode) {
    if (fft_size < 4 || width < 2 || width > design::kViewMaxSide || height < 1 || height > design::kViewMaxSide ||
        (mode != CSDR_WF_VIEW_LINEAR && mode != CSDR_WF_VIEW_PEAK))
        return fail(CSDR_EINVAL, "view %d x %d, mode %d of fft_size %d (fft_size >= 4, width 2 .. 16384, height 1 .. 16384)", width, height, mode, fft_size);
    return CSDR_OK;
}

// the `lines` rows of one ring texture to the host, dense; ends in a synchronise
inline int wf_fetch_rows(hipStream_t st, const uint8_t *src, int lines, int half, int pitch, uint8_t *out_u8) {
    if (pitch == half) CSDR_HIP_TRY(hipMemcpyAsync(out_u8, src, (size_t)lines * half, hipMemcpyDeviceToHost, st));
    else for (int r = 0; r < lines; ++r)
        CSDR_HIP_TRY(hipMemcpyAsync(out_u8 + (size_t)r * half, src + (size_t)r * pitch, (size_t)half, hipMemcpyDeviceToHost, st));
    CSDR_HIP_TRY(hipStreamSynchronize(st));
    return CSDR_OK;
}

// the 256-entry RGBA8 colour table: upload, and what it holds before any set_gradient: i -> (i, i, i, 255)
inline int wf_upload_table(hipStream_t st, uint32_t *table, const uint32_t *t) {
    CSDR_HIP_TRY(hipMemcpyAsync(table, t, 256 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    CSDR_HIP_TRY(hipStreamSynchronize(st));              // (t is the caller's stack)
    return CSDR_OK;
}
inline int wf_upload_grey_table(hipStream_t st, uint32_t *table) {
    uint32_t grey[256];
    for (uint32_t i = 0; i < 256; ++i) grey[i] = i | (i << 8) | (i << 16) | 0xff000000u;
    return wf_upload_table(st, table, grey);
}

// 2 fft_size floats: the (x, y) pairs of SpectrumVisualData (:40-45); fft_size floats: as they stand (:47); anything else leaves the points alone
// (WaterfallCanvas.cpp:106-109) and the step repeats them
inline bool wf_line_is_pairs(int n_floats_per_line, int fft_size) { return n_floats_per_line == 2 * fft_size; }
inline bool wf_good_line(const float *points, int n_floats_per_line, int fft_size) {
    return points && (wf_line_is_pairs(n_floats_per_line, fft_size) || n_floats_per_line == fft_size);
}

}  // namespace csdr
