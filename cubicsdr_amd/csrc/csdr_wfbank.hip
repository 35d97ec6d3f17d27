// csdr_wfbank.hip -- implementation of include/csdr_hip.h (gfx950): csdr_wfbank, N independent WaterfallPanels (src/panel/WaterfallPanel.cpp) of one
// fft_size and one `lines` whose pending lines, kept points, ring textures and pictures stay in HBM.  The host keeps every slot's integers -- the
// offset, lines_buffered, whether the textures exist -- exactly as csdr_waterfall.hip keeps one panel's, plans a call from them and uploads the plan
// as records; ONE launch (kernels_wfbank.hpp) then moves the bytes of all slots: one per step, step_specbank, update and render, whatever the
// number of slots, items and runs.  All work runs on a stream of the object's own; a spectrum bank's points are reached through
// specbank_points_acquire / _release (csdr_objects.hpp), ordered by events.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#define CSDR_TU_WFBANK 1     // this unit is the home of its kernels (kernels_wfbank.hpp)
#include "csdr_objects.hpp"
#include "kernels_wfbank.hpp"
#include "waterfall_host.hpp"

using namespace csdr;

static_assert(sizeof(csdr_wfbank_item) == 24 && offsetof(csdr_wfbank_item, points) == 8 && offsetof(csdr_wfbank_item, is_dev) == 16 &&
              offsetof(csdr_wfbank_item, n_lines) == 20, "csdr_wfbank_item layout");

namespace {
// WaterfallPanel's state, per slot
struct WbSlot {
    int lines_buffered = 0;                            // lines_buffered (:16, :81, :157)
    bool buffer_init = false, tex_init = false;        // bufferInitialized, texInitialized (:22-23)
    int ofs = 0;                                       // waterfall_ofs (both halves move together: they start equal)
    int par = 0;                                       // which of the slot's two copies of `points` is current
    bool has_points = false;                           // a line was kept since the points were last zero
};
// a slot's scratch while a step is planned
struct WbPlan {
    int added = 0;                                     // lines the call stores for the slot
    const float *cur = nullptr;                        // the slot's last good line of the call where the device reads it; nullptr: the kept points
    int cur_flags = 0;
    int keep_job = -1;                                 // the job of that line
    const float *drop = nullptr;                       // a slot without textures: its last good line (host or device memory as given)
    int drop_nf = 0, drop_dev = 0;
    bool touched = false;
};
constexpr int kWbStage = 2;                            // page-locked staging sets of the records
constexpr int kWbPeakRows = 8;                         // wfb_view_peak: image rows to a workgroup at most (16 KB of LDS at half 2048)
}  // namespace

struct csdr_wfbank : SideStream {                      // (ev_in: device lines of the caller; ev_out: csdr_wfbank_device_view)
    bool ready = false;
    int fft_size = 0, half = 0, pitch = 0, lines = 0, max_slots = 0, max_pending = 0;
    int fp = 0;                                        // floats of one copy of a slot's points: fft_size rounded up to 16 bytes
    std::vector<WbSlot> slots;
    DevBuf<float> points;                              // [max_slots][2 copies][fp]
    DevBuf<uint8_t> pend, ring;                        // lineBuffer[2] per slot: [max_slots][2][max_pending][pitch]; the textures: [max_slots][2][lines][pitch]
    DevBuf<uint32_t> table, view;                      // the 256-entry RGBA8 table; the last rendered atlas
    WfTapCache taps;                                   // one pair of tables for all slots: they share fft_size and lines
    int view_w = 0, view_h = 0;                        // the last rendered atlas in pixels; 0: none
    StageRing<kWbStage> plan;                          // the records of the call being run (and the staged host lines of a step behind them)
    // scratch of a call's planning
    std::vector<WbPlan> work;
    std::vector<int> touched;
    std::vector<csdr_wfbank_item> sb_items;
    std::vector<int> sb_taken;
    int64_t pend_half() const { return (int64_t)max_pending * pitch; }
    int64_t ring_half() const { return (int64_t)lines * pitch; }
    float *points_of(int slot, int copy) const { return points.p + ((size_t)slot * 2 + (size_t)copy) * (size_t)fp; }
    uint8_t *ring_of(int slot, int j) const { return ring.p + ((size_t)slot * 2 + (size_t)j) * (size_t)ring_half(); }
};

#define WFB_LAUNCH(w_, kid_, kern_, grid_, block_, lds_, ...) \
    do { ProfScope ps__((w_)->ctx, (kid_), (w_)->st); hipLaunchKernelGGL(kern_, grid_, dim3((unsigned)(block_)), lds_, (w_)->st, __VA_ARGS__); } while (0)

// the workgroup for `items` work-items of a row: whole waves, 256 work-items at most
static int wb_block(int items) { return std::min(kWfThreads, (items + 63) / 64 * 64); }

extern "C" int csdr_wfbank_create(csdr_ctx *ctx, csdr_wfbank **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    std::unique_ptr<csdr_wfbank, void (*)(csdr_wfbank *)> w(new csdr_wfbank(), csdr_wfbank_destroy);
    if (int rc = w->create(ctx)) return rc;
    if (int rc = w->plan.create()) return rc;
    if (int rc = w->table.reserve(256)) return rc;
    if (int rc = wf_upload_grey_table(w->st, w->table.p)) return rc;        // before any csdr_wfbank_set_gradient
    *out = w.release();
    return CSDR_OK;
}

extern "C" void csdr_wfbank_destroy(csdr_wfbank *w) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w) return;
    w->destroy();
    w->plan.destroy();
    w->points.release(); w->pend.release(); w->ring.release(); w->table.release(); w->view.release(); w->taps.dev.release();
    delete w;
}

// WaterfallPanel::setup (:13-24) on every slot
extern "C" int csdr_wfbank_setup(csdr_wfbank *w, int fft_size, int lines, int max_slots, int max_pending) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w) return fail(CSDR_EINVAL, "waterfall bank is null");
    if (fft_size < 2 || fft_size > 4096) return fail(CSDR_EINVAL, "fft_size %d: 2 .. 4096", fft_size);
    // (with one line waterfall_ofs starts at 0, the first run has no rows and the loop of :140-158 never ends)
    if (lines < 2 || lines > 4096) return fail(CSDR_EINVAL, "lines %d: 2 .. 4096", lines);
    if (max_slots < 1 || max_slots > 4096) return fail(CSDR_EINVAL, "max_slots %d: 1 .. 4096", max_slots);
    if (max_pending < 1 || max_pending > (1 << 20)) return fail(CSDR_EINVAL, "max_pending %d: 1 .. 2^20", max_pending);
    CSDR_HIP_TRY(hipStreamSynchronize(w->st));
    const int half = fft_size / 2, pitch = (half + 15) / 16 * 16, fp = (fft_size + 3) / 4 * 4;
    w->ready = false;
    if (fft_size != w->fft_size || max_slots != w->max_slots) {
        // points.resize(fft_size) (:18-20) per slot: the values in front stay, new ones are zero; a slot the object did not have is a new panel
        DevBuf<float> np;
        const size_t n = (size_t)max_slots * 2 * (size_t)fp;
        if (int rc = np.reserve(n)) return rc;
        CSDR_HIP_TRY(hipMemsetAsync(np.p, 0, n * sizeof(float), w->st));
        std::vector<WbSlot> ns((size_t)max_slots);
        for (int s = 0; s < std::min(max_slots, w->max_slots); ++s) {
            const WbSlot &o = w->slots[(size_t)s];
            if (!o.has_points) continue;
            CSDR_HIP_TRY(hipMemcpyAsync(np.p + (size_t)s * 2 * (size_t)fp, w->points_of(s, o.par), (size_t)std::min(fft_size, w->fft_size) * sizeof(float),
                                        hipMemcpyDeviceToDevice, w->st));
            ns[(size_t)s].has_points = true;             // (copy 0 is current)
        }
        CSDR_HIP_TRY(hipStreamSynchronize(w->st));
        w->points.release();
        w->points = np;
        w->slots.swap(ns);
    }
    if (int rc = w->pend.reserve((size_t)max_slots * 2 * (size_t)max_pending * (size_t)pitch)) return rc;
    if (int rc = w->ring.reserve((size_t)max_slots * 2 * (size_t)lines * (size_t)pitch)) return rc;
    // (the rows' padding is copied along by wfb_update and read by wfb_view_peak: it is zero and stays zero, no kernel writes it)
    CSDR_HIP_TRY(hipMemsetAsync(w->pend.p, 0, (size_t)max_slots * 2 * (size_t)max_pending * (size_t)pitch, w->st));
    w->fft_size = fft_size; w->half = half; w->pitch = pitch; w->fp = fp; w->lines = lines; w->max_slots = max_slots; w->max_pending = max_pending;
    for (WbSlot &s : w->slots) {
        s.lines_buffered = 0;                            // :16
        s.tex_init = s.buffer_init = false;              // :22-23
        s.ofs = 0;
    }
    w->work.assign((size_t)max_slots, WbPlan());
    w->touched.clear();
    w->taps.forget(); w->view_w = w->view_h = 0;
    w->ready = true;
    return CSDR_OK;
}

// refreshTheme (:26-37): one table for all slots
extern "C" int csdr_wfbank_set_gradient(csdr_wfbank *w, const float *rgb_stops, int n_colors) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w) return fail(CSDR_EINVAL, "waterfall bank is null");
    uint32_t t[256];
    if (!design::gradient_rgba8(rgb_stops, n_colors, t)) return fail(CSDR_EINVAL, "gradient: %d stops (2 .. 257, no null pointer)", n_colors);
    return wf_upload_table(w->st, w->table.p, t);
}

extern "C" int csdr_wfbank_reset_slot(csdr_wfbank *w, int slot) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !w->ready) return fail(CSDR_ESTATE, "waterfall bank not set up");
    if (slot < 0 || slot >= w->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, w->max_slots);
    WbSlot &s = w->slots[(size_t)slot];
    if (s.has_points) CSDR_HIP_TRY(hipMemsetAsync(w->points_of(slot, 0), 0, 2 * (size_t)w->fp * sizeof(float), w->st));
    s = WbSlot();
    return CSDR_OK;
}

// setPoints (:39-49) + step (:51-83) for every line of every item; `items` are checked.  from_boundary: device lines were produced on the boundary
// stream (the public call); otherwise the caller has ordered them already (a spectrum bank's points)
static int wb_step(csdr_wfbank *w, const csdr_wfbank_item *items, int n_items, int *taken, bool from_boundary) {
    if (taken) for (int i = 0; i < n_items; ++i) taken[i] = 0;
    const int F = w->fft_size;
    auto good = [F](const csdr_wfbank_item &it) { return wf_good_line(it.points, it.n_floats_per_line, F); };       // (else the step repeats the points)
    auto forget = [w]() { for (int s : w->touched) w->work[(size_t)s] = WbPlan(); w->touched.clear(); };
    // ---- count: a refused call leaves every slot as it was
    size_t n_jobs = 0, host_floats = 0;
    bool any_dev = false;
    for (int i = 0; i < n_items; ++i) {
        const csdr_wfbank_item &it = items[i];
        if (it.n_lines == 0) continue;
        const WbSlot &sl = w->slots[(size_t)it.slot];
        WbPlan &p = w->work[(size_t)it.slot];
        if (!p.touched) { p.touched = true; w->touched.push_back(it.slot); }
        const bool ok = good(it);
        const size_t line = ((size_t)it.n_floats_per_line + 3) / 4 * 4;          // a staged line starts on a 16-byte boundary
        if (sl.tex_init) {
            p.added += it.n_lines;
            if (sl.lines_buffered + (int64_t)p.added > w->max_pending) {
                const int have = sl.lines_buffered, add = p.added;
                forget();
                return fail(CSDR_ERANGE, "slot %d: %d pending lines + %d exceed max_pending %d", it.slot, have, add, w->max_pending);
            }
            n_jobs += (size_t)it.n_lines;
            if (ok && !it.is_dev) host_floats += (size_t)it.n_lines * line;
        } else if (ok) {                                  // :60-62: dropped, but setPoints has run -- the slot's last good line is kept
            if (!p.drop) ++n_jobs;
            p.drop = it.points + (size_t)(it.n_lines - 1) * (size_t)it.n_floats_per_line;
            p.drop_nf = it.n_floats_per_line; p.drop_dev = it.is_dev;
            if (!it.is_dev) host_floats += line;          // (room for every candidate; only the last is staged)
        }
        if (ok && it.is_dev) any_dev = true;
    }
    for (int s : w->touched) w->work[(size_t)s].added = 0;
    // ---- from here on the call cannot be refused
    for (int s : w->touched) w->slots[(size_t)s].buffer_init = true;             // :54-58
    if (n_jobs == 0) { forget(); return CSDR_OK; }       // steps without points on slots without textures: nothing to quantise, nothing to keep
    const size_t lines_at = n_jobs * sizeof(WfbJob), bytes = lines_at + host_floats * sizeof(float);
    if (int rc = w->plan.begin(w->st, bytes)) { forget(); return rc; }
    if (any_dev && from_boundary) if (int rc = w->after_boundary()) return rc;  // the caller produced them on the boundary stream
    WfbJob *jobs = reinterpret_cast<WfbJob *>(w->plan.host());
    float *stage_h = reinterpret_cast<float *>(w->plan.host() + lines_at);
    const float *stage_d = reinterpret_cast<const float *>(w->plan.device() + lines_at);
    size_t nj = 0, at = 0;
    const bool wide_ok = w->half % 16 == 0;
    auto line_flags = [wide_ok](const float *dev, bool pair) { return (pair ? kWfbPair : 0) | (wide_ok && ((uintptr_t)dev & 15) == 0 ? kWfbWide : 0); };
    auto stage_line = [&](const float *host, int nf) {   // -> where the device reads the copy
        memcpy(stage_h + at, host, (size_t)nf * sizeof(float));
        const float *d = stage_d + at;
        at += ((size_t)nf + 3) / 4 * 4;
        return d;
    };
    for (int i = 0; i < n_items; ++i) {
        const csdr_wfbank_item &it = items[i];
        if (it.n_lines == 0) continue;
        const WbSlot &sl = w->slots[(size_t)it.slot];
        WbPlan &p = w->work[(size_t)it.slot];
        if (!sl.tex_init) continue;
        const bool ok = good(it), pair = wf_line_is_pairs(it.n_floats_per_line, F);
        for (int l = 0; l < it.n_lines; ++l) {
            WfbJob jb{};
            jb.slot = it.slot; jb.row = sl.lines_buffered + p.added++;
            if (ok) {
                const float *src = it.points + (size_t)l * (size_t)it.n_floats_per_line;
                jb.src = it.is_dev ? src : stage_line(src, it.n_floats_per_line);
                jb.flags = line_flags(jb.src, pair);
                p.cur = jb.src; p.cur_flags = jb.flags; p.keep_job = (int)nj;
            } else if (p.cur) { jb.src = p.cur; jb.flags = p.cur_flags; }            // the good line in front of it in this call
            else { jb.src = w->points_of(it.slot, sl.par); jb.flags = line_flags(jb.src, false); }      // the points kept before the call
            jobs[nj++] = jb;
        }
        if (taken) taken[i] = it.n_lines;                // :81
    }
    for (int s : w->touched) {
        WbSlot &sl = w->slots[(size_t)s];
        WbPlan &p = w->work[(size_t)s];
        if (!sl.tex_init && p.drop) {
            WfbJob jb{};
            jb.slot = s; jb.row = -1;
            jb.src = p.drop_dev ? p.drop : stage_line(p.drop, p.drop_nf);
            jb.flags = line_flags(jb.src, wf_line_is_pairs(p.drop_nf, F));
            p.keep_job = (int)nj;
            jobs[nj++] = jb;
        }
        if (p.keep_job >= 0) {                           // the call's last good line becomes the slot's points: into the copy nothing reads
            jobs[p.keep_job].keep = w->points_of(s, sl.par ^ 1);
            sl.par ^= 1;
            sl.has_points = true;
        }
        sl.lines_buffered += p.added;
    }
    forget();
    if (int rc = w->plan.uploaded(w->st, lines_at + at * sizeof(float))) return rc;
    WfbQuantArgs a{};
    a.jobs = reinterpret_cast<const WfbJob *>(w->plan.device()); a.n_jobs = (int)nj;
    a.half = w->half; a.pitch = w->pitch; a.pend = w->pend.p; a.pend_half = w->pend_half();
    const int items_x = (w->half + kWfChunk - 1) / kWfChunk, block = wb_block(items_x);
    const dim3 grid((unsigned)((items_x + block - 1) / block), (unsigned)std::min<size_t>(nj, 65535), 2);
    WFB_LAUNCH(w, KID_WFB_QUANTIZE, wfb_quantize, grid, block, 0, a);
    CSDR_HIP_TRY(hipGetLastError());
    return CSDR_OK;
}

static int wb_check_items(const csdr_wfbank *w, const csdr_wfbank_item *items, int n_items) {
    if (n_items < 0 || (n_items > 0 && !items)) return fail(CSDR_EINVAL, "bad items");
    for (int i = 0; i < n_items; ++i) {
        const csdr_wfbank_item &it = items[i];
        if (it.slot < 0 || it.slot >= w->max_slots) return fail(CSDR_EINVAL, "item %d: slot %d of %d", i, it.slot, w->max_slots);
        if (it.n_lines < 0 || it.n_floats_per_line < 0) return fail(CSDR_EINVAL, "item %d: bad line arguments", i);
        if (it.points && it.is_dev && ((uintptr_t)it.points & 3)) return fail(CSDR_EINVAL, "item %d: device points must be 4-byte aligned", i);
    }
    return CSDR_OK;
}

extern "C" int csdr_wfbank_step(csdr_wfbank *w, const csdr_wfbank_item *items, int n_items, int *taken) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !w->ready) return fail(CSDR_ESTATE, "waterfall bank not set up");
    if (taken) for (int i = 0; i < n_items; ++i) taken[i] = 0;
    if (int rc = wb_check_items(w, items, n_items)) return rc;
    return wb_step(w, items, n_items, taken, true);
}

extern "C" int csdr_wfbank_step_specbank(csdr_wfbank *w, csdr_specbank *sb, int *taken_total) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (taken_total) *taken_total = 0;
    if (!w || !w->ready) return fail(CSDR_ESTATE, "waterfall bank not set up");
    if (!sb) return fail(CSDR_EINVAL, "spectrum bank is null");
    SpecBankPointsRef ref;
    if (int rc = specbank_points_acquire(sb, w->st, &ref)) return rc;
    if (ref.ctx != w->ctx) return fail(CSDR_EINVAL, "the spectrum bank belongs to another context");
    // a spectrum bank of another size delivers frames of the wrong size (WaterfallCanvas.cpp:106-109): the previous points are stepped
    const bool same = ref.F == w->fft_size;
    w->sb_items.clear();
    const int ns = std::min(w->max_slots, ref.max_slots);
    for (int s = 0; s < ns; ++s) {
        const int f = csdr_specbank_frames(sb, s);
        if (f > 0) w->sb_items.push_back(csdr_wfbank_item{s, ref.F, same ? ref.points + (size_t)s * (size_t)ref.max_frames * (size_t)ref.F : nullptr, 1, f});
    }
    w->sb_taken.assign(w->sb_items.size(), 0);
    const int rc = wb_step(w, w->sb_items.data(), (int)w->sb_items.size(), w->sb_taken.data(), false);
    if (int r2 = specbank_points_release(sb, w->st)) return r2;
    if (rc == CSDR_OK && taken_total) for (int t : w->sb_taken) *taken_total += t;
    return rc;
}

// WaterfallPanel::update (:85-159) on every slot
extern "C" int csdr_wfbank_update(csdr_wfbank *w) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !w->ready) return fail(CSDR_ESTATE, "waterfall bank not set up");
    size_t n_upd = 0;
    for (const WbSlot &s : w->slots) if (s.buffer_init && s.lines_buffered > 0) ++n_upd;
    if (n_upd) if (int rc = w->plan.begin(w->st, n_upd * sizeof(WfbUpdate))) return rc;
    WfbUpdate *upd = n_upd ? reinterpret_cast<WfbUpdate *>(w->plan.host()) : nullptr;
    size_t nu = 0;
    int rows_max = 0, fill0 = -1;                        // fill0: first slot of a run of neighbours whose textures are being created
    const size_t slot_bytes = 2 * (size_t)w->ring_half();
    for (int si = 0; si <= w->max_slots; ++si) {
        WbSlot *s = si < w->max_slots ? &w->slots[(size_t)si] : nullptr;
        const bool create = s && s->buffer_init && !s->tex_init;          // :88-90, :92-130: both textures zero-filled, waterfall_ofs = lines - 1
        if (create && fill0 < 0) fill0 = si;
        if (!create && fill0 >= 0) {                     // one fill for the whole run of neighbours
            CSDR_HIP_TRY(hipMemsetAsync(w->ring_of(fill0, 0), 0, (size_t)(si - fill0) * slot_bytes, w->st));
            fill0 = -1;
        }
        if (!s || !s->buffer_init) continue;
        if (create) { s->ofs = w->lines - 1; s->tex_init = true; }
        const int n = s->lines_buffered;
        if (n == 0) continue;
        const WfUpdatePlan plan = wf_plan_update(s->ofs, w->lines, n);           // :139-158
        WfbUpdate u{};
        u.slot = si; u.n_pending = n; u.n_runs = plan.n_runs;
        u.run[0] = plan.run[0]; u.run[1] = plan.run[1];
        rows_max = std::max(rows_max, plan.rows());
        upd[nu++] = u;
        s->ofs = plan.ofs;
        s->lines_buffered = 0;
    }
    if (nu == 0) return CSDR_OK;
    if (int rc = w->plan.uploaded(w->st, nu * sizeof(WfbUpdate))) return rc;
    WfbUpdateArgs a{};
    a.upd = reinterpret_cast<const WfbUpdate *>(w->plan.device());
    a.pitch = w->pitch; a.ring = w->ring.p; a.pend = w->pend.p; a.ring_half = w->ring_half(); a.pend_half = w->pend_half();
    const int chunks = w->pitch / 16, block = wb_block(chunks);
    const dim3 grid((unsigned)((chunks + block - 1) / block), (unsigned)std::min(rows_max, 65535), (unsigned)(2 * nu));
    WFB_LAUNCH(w, KID_WFB_UPDATE, wfb_update, grid, block, 0, a);
    CSDR_HIP_TRY(hipGetLastError());
    return CSDR_OK;
}

extern "C" int csdr_wfbank_lines_buffered(const csdr_wfbank *w, int slot) {
    return w && w->ready && slot >= 0 && slot < w->max_slots ? w->slots[(size_t)slot].lines_buffered : 0;
}
extern "C" int csdr_wfbank_offset(const csdr_wfbank *w, int slot, int half) {
    return w && w->ready && slot >= 0 && slot < w->max_slots && w->slots[(size_t)slot].tex_init && (half == 0 || half == 1) ? w->slots[(size_t)slot].ofs : -1;
}

extern "C" int csdr_wfbank_fetch_index(csdr_wfbank *w, int slot, int half, uint8_t *out_u8, int64_t cap) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !w->ready) return fail(CSDR_ESTATE, "waterfall bank not set up");
    if (slot < 0 || slot >= w->max_slots || (half != 0 && half != 1) || !out_u8) return fail(CSDR_EINVAL, "bad argument");
    if (!w->slots[(size_t)slot].tex_init) return fail(CSDR_ESTATE, "slot %d: no textures yet (setup, step, update)", slot);
    if (cap < (int64_t)w->lines * w->half) return fail(CSDR_ERANGE, "need %lld bytes", (long long)w->lines * w->half);
    return wf_fetch_rows(w->st, w->ring_of(slot, half), w->lines, w->half, w->pitch, out_u8);
}

// drawPanelContents (:161-219) of every listed slot, scaled to width x height, as one atlas
extern "C" int csdr_wfbank_render(csdr_wfbank *w, const int *slots, int n_slots, int width, int height, int mode, int atlas_cols, uint8_t *out_u8, int64_t cap) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !w->ready) return fail(CSDR_ESTATE, "waterfall bank not set up");
    if (int rc = wf_check_view(w->fft_size, width, height, mode)) return rc;
    if (n_slots < 1 || n_slots > (1 << 20)) return fail(CSDR_EINVAL, "n_slots %d: 1 .. 2^20", n_slots);
    if (atlas_cols < 1 || atlas_cols > n_slots) return fail(CSDR_EINVAL, "atlas_cols %d: 1 .. n_slots (%d)", atlas_cols, n_slots);
    if (slots) for (int i = 0; i < n_slots; ++i) if (slots[i] < 0 || slots[i] >= w->max_slots) return fail(CSDR_EINVAL, "entry %d: slot %d of %d", i, slots[i], w->max_slots);
    if (!slots && n_slots > w->max_slots) return fail(CSDR_EINVAL, "slots 0 .. %d of %d", n_slots - 1, w->max_slots);
    const int tile_rows = (n_slots + atlas_cols - 1) / atlas_cols;
    const int64_t n_tiles = (int64_t)tile_rows * atlas_cols;
    const int64_t pic_w = (int64_t)atlas_cols * width, pic_h = (int64_t)tile_rows * height, pixels = pic_w * pic_h;
    const int groups = (width + 3) / 4, per_tile = (int)(((int64_t)groups * height + kWfThreads - 1) / kWfThreads);
    if (pic_w > 0x7fffffff || pic_h > 0x7fffffff || n_tiles * per_tile > 0x7fffffff) return fail(CSDR_EINVAL, "an atlas of %lld x %lld pixels", (long long)pic_w, (long long)pic_h);
    if (out_u8 && cap < 4 * pixels) return fail(CSDR_ERANGE, "need %lld bytes", (long long)(4 * pixels));
    if (int rc = w->taps.ensure(w->st, w->fft_size, w->lines, width, height, mode)) return rc;
    if ((size_t)pixels > w->view.cap) {
        CSDR_HIP_TRY(hipStreamSynchronize(w->st));
        w->view_w = w->view_h = 0;                       // (the buffer csdr_wfbank_device_view handed out goes away)
    }
    if (int rc = w->view.reserve((size_t)pixels)) return rc;
    if (int rc = w->plan.begin(w->st, (size_t)n_tiles * sizeof(WfbTile))) return rc;
    WfbTile *tiles = reinterpret_cast<WfbTile *>(w->plan.host());
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int s = t < n_slots ? (slots ? slots[t] : (int)t) : -1;
        tiles[t] = WfbTile{std::max(s, 0), s >= 0 && w->slots[(size_t)s].tex_init ? w->slots[(size_t)s].ofs : -1};       // :162-164 per slot: nothing is drawn
    }
    if (int rc = w->plan.uploaded(w->st, (size_t)n_tiles * sizeof(WfbTile))) return rc;
    WfbViewArgs a{};
    a.tiles = reinterpret_cast<const WfbTile *>(w->plan.device());
    a.ring = w->ring.p; a.ring_half = w->ring_half(); a.table = w->table.p;
    a.cols = w->taps.dev.p; a.rows = w->taps.dev.p + width; a.out = w->view.p;
    a.width = width; a.height = height; a.pitch = w->pitch; a.lines = w->lines; a.atlas_cols = atlas_cols;
    if (mode == CSDR_WF_VIEW_LINEAR) {
        a.groups = groups; a.per_tile = per_tile;
        WFB_LAUNCH(w, KID_WFB_VIEW_LINEAR, wfb_view_linear, dim3((unsigned)(n_tiles * per_tile)), kWfThreads, 256 * sizeof(uint32_t), a);
    } else {
        // as many image rows to a workgroup as give every work-item a pixel of the wider half, kWbPeakRows at most
        a.n0 = width / 2; a.chunks = w->pitch / 16;
        a.rows_per = std::max(1, std::min(std::min(height, kWbPeakRows), kWfThreads / (width - a.n0)));
        const dim3 grid((unsigned)n_tiles, (unsigned)((height + a.rows_per - 1) / a.rows_per), 2);
        WFB_LAUNCH(w, KID_WFB_VIEW_PEAK, wfb_view_peak, grid, kWfThreads, 256 * sizeof(uint32_t) + (size_t)a.rows_per * (size_t)a.chunks * 16, a);
    }
    CSDR_HIP_TRY(hipGetLastError());
    w->view_w = (int)pic_w; w->view_h = (int)pic_h;
    if (out_u8) {
        CSDR_HIP_TRY(hipMemcpyAsync(out_u8, w->view.p, (size_t)(4 * pixels), hipMemcpyDeviceToHost, w->st));
        CSDR_HIP_TRY(hipStreamSynchronize(w->st));
    }
    return CSDR_OK;
}

extern "C" int csdr_wfbank_device_view(csdr_wfbank *w, const uint8_t **dev, int *pic_width, int *pic_height) {
    DeviceScope dev__(w ? w->ctx : nullptr);
    if (!w || !dev) return fail(CSDR_EINVAL, "null argument");
    if (!w->ready || w->view_w == 0) return fail(CSDR_ESTATE, "nothing rendered yet (csdr_wfbank_render)");
    if (int rc = w->hand_over()) return rc;
    *dev = reinterpret_cast<const uint8_t *>(w->view.p);
    if (pic_width) *pic_width = w->view_w;
    if (pic_height) *pic_height = w->view_h;
    return CSDR_OK;
}
