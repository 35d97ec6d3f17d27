// csdr_ctx.hip -- implementation of include/csdr_hip.h (gfx950): context, streams, profiling hooks, device memory helpers.  Host-side bookkeeping mirrors the reference's control flow
// (file:line cited per function); all sample arithmetic is in the kernels_*.hpp kernels.
#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <map>
#include <memory>

#include "common.hpp"
#include "design.hpp"

#include <dlfcn.h>

using namespace csdr;

namespace csdr {
Roctx &roctx() { static Roctx r; return r; }
static void roctx_load_once() {
    static std::once_flag once;
    std::call_once(once, [] {
        const char *e = getenv("CSDR_ROCTX");
        if (!e || atoi(e) == 0) return;
        for (const char *name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            void *h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (!h) continue;
            Roctx &r = roctx();
            *(void **)(&r.push) = dlsym(h, "roctxRangePushA");
            *(void **)(&r.pop) = dlsym(h, "roctxRangePop");
            if (r.push && r.pop) return;
            r.push = nullptr; r.pop = nullptr;
            dlclose(h);
        }
    });
}
}  // namespace csdr

// =================================================================================================== context
extern "C" int csdr_abi_version(void) { return 1; }

extern "C" const char *csdr_strerror(int code) {
    switch (code) {
        case CSDR_OK: return "ok";
        case CSDR_EINVAL: return "invalid argument";
        case CSDR_ENOMEM: return "out of memory";
        case CSDR_EHIP: return "HIP runtime error";
        case CSDR_ESTATE: return "object not configured";
        case CSDR_ERANGE: return "capacity exceeded";
        case CSDR_EUNSUPPORTED: return "not supported yet";
        default: return "unknown error";
    }
}
extern "C" const char *csdr_last_error(void) { return last_error_ref().c_str(); }

extern "C" int csdr_ctx_create(int device, void *hip_stream, csdr_ctx **out) {
    if (!out) return fail(CSDR_EINVAL, "out is null");
    *out = nullptr;
    roctx_load_once();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(CSDR_EHIP, "no HIP device available: the HIP path cannot run (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(CSDR_EINVAL, "device %d out of range (%d devices)", device, ndev);
    CSDR_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<csdr_ctx> c(new csdr_ctx());
    c->device = device;
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cu < 1) c->n_cu = 256;
    // Physical streams.  The five stage lanes are folded onto three streams by default: channelizer | demodulators | spectrum
    // (the reference's own cut: SDRPostThread, the demodulator threads, the spectrum thread), so that the channelizer of batch
    // n + 1 runs next to the demodulators of batch n.  Measured on MI355X / ROCm 7.2, C3: 1 / 2 / 3 / 5 streams = 51.0 / 50.9 /
    // 52.8 / 52.3 GS/s at 128-block batches and 5.8 / 7.9 / 9.3 / 8.9 thousand one-block calls per second.  CSDR_STREAMS = 1 | 2 |
    // 3 | 5 selects a folding (2: {channelizer + demodulators} | {spectrum}; 5: one stream per stage); the event protocol is the
    // same for all.
    int want = 3;
    if (const char *e = getenv("CSDR_STREAMS")) want = atoi(e);
    if (want != 1 && want != 2 && want != 3 && want != 5) want = 3;
    static const int kMap[6][LANE_COUNT] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 1, 1}, {0, 1, 1, 2, 2}, {0, 0, 0, 0, 0}, {0, 1, 2, 3, 4}};
    c->n_phys = want;
    for (int l = 0; l < want; ++l) {
        CSDR_HIP_TRY(hipStreamCreateWithFlags(&c->phys[l], hipStreamNonBlocking));
        CSDR_HIP_TRY(hipEventCreateWithFlags(&c->ev_lane[l], hipEventDisableTiming));
    }
    for (int l = 0; l < LANE_COUNT; ++l) c->lanes[l] = c->phys[kMap[want][l]];
    if (hip_stream == CSDR_STREAM_NULL) { c->stream = nullptr; c->own_stream = false; }          // the device's null stream
    else if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->own_stream = false; }
    else { c->stream = c->phys[0]; c->own_stream = true; }      // a private boundary stream is just the first stage stream
    for (int l = 0; l < LANE_COUNT; ++l) CSDR_HIP_TRY(hipEventCreateWithFlags(&c->ev_in[l], hipEventDisableTiming));
    CSDR_HIP_TRY(hipEventCreate(&c->ev0));
    CSDR_HIP_TRY(hipEventCreate(&c->ev1));
    std::vector<float> tab = design::nco_sine_table();
    if (int rc = c->sintab.reserve(1024)) return rc;
    CSDR_HIP_TRY(hipMemcpy(c->sintab.p, tab.data(), 1024 * sizeof(float), hipMemcpyHostToDevice));
    *out = c.release();
    return CSDR_OK;
}
extern "C" void csdr_ctx_destroy(csdr_ctx *c) {
    DeviceScope dev__(c);
    if (!c) return;
    (void)c->sync_all();
    c->sintab.release();
    for (auto &r : c->prof_pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : c->prof_pool) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (int l = 0; l < LANE_COUNT; ++l) if (c->ev_in[l]) (void)hipEventDestroy(c->ev_in[l]);
    for (int l = 0; l < c->n_phys; ++l) {
        if (c->ev_lane[l]) (void)hipEventDestroy(c->ev_lane[l]);
        if (c->phys[l]) (void)hipStreamDestroy(c->phys[l]);
    }
    delete c;
}
extern "C" int csdr_ctx_synchronize(csdr_ctx *c) {
    DeviceScope dev__(c);
    if (!c) return fail(CSDR_EINVAL, "ctx is null");
    return c->sync_all();
}
extern "C" int csdr_ctx_join(csdr_ctx *c) {
    DeviceScope dev__(c);
    if (!c) return fail(CSDR_EINVAL, "ctx is null");
    return c->join();
}
extern "C" int csdr_ctx_owns_stream(const csdr_ctx *c) { return c && c->own_stream ? 1 : 0; }
extern "C" void *csdr_ctx_stream(csdr_ctx *c) { return c ? (void *)c->stream : nullptr; }
extern "C" int csdr_ctx_timer_start(csdr_ctx *c) {
    DeviceScope dev__(c);
    if (!c) return fail(CSDR_EINVAL, "ctx is null");
    if (int rc = c->join()) return rc;
    CSDR_HIP_TRY(hipEventRecord(c->ev0, c->stream));
    // nothing the stage streams receive from now on may start before the timer's start mark
    for (int l = 0; l < c->n_phys; ++l) if (c->phys[l] != c->stream) CSDR_HIP_TRY(hipStreamWaitEvent(c->phys[l], c->ev0, 0));
    return CSDR_OK;
}
extern "C" int csdr_ctx_timer_stop(csdr_ctx *c, float *ms) {
    DeviceScope dev__(c);
    if (!c || !ms) return fail(CSDR_EINVAL, "null argument");
    if (int rc = c->join()) return rc;
    CSDR_HIP_TRY(hipEventRecord(c->ev1, c->stream));
    CSDR_HIP_TRY(hipEventSynchronize(c->ev1));
    CSDR_HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return CSDR_OK;
}
// ---- per-kernel HIP-event profile (bench.py roofline leg) ----
static const char *kKernelNames[KID_COUNT] = {
    "chan_analyze", "dc_tile_ends", "dc_apply", "rows_copy",
    "demod_frontend_generic", "demod_frontend_s3", "demod_frontend_s4", "demod_frontend_s5", "demod_frontend_s6", "demod_frontend_s56", "demod_frontend_interp",
    "demod_modem", "demod_gain_scan", "fms_stages", "demod_audio_interp", "fms_out", "audio_egress", "bank_tables",
    "spec_fft_radix", "spec_fft_rows", "spec_average", "spec_extrema", "spec_display", "spec_misc",
    "digital_demod",
    "wf_quantize", "wf_update", "wf_rgba", "wf_view_linear", "wf_view_peak",
    "distrib_gather",
    "specbank_process",
    "wfb_quantize", "wfb_update", "wfb_view_linear", "wfb_view_peak",
    "scopebank_wave", "scopebank_spectrum",
    "squelch_scan", "squelch_pack", "squelch_pcm16",
    "viewbank_process",
    "trace_lines", "trace_xy",
    "overlay_compose",
    "density_cover", "density_fold", "density_render"};
static int prof_drain(csdr_ctx *c) {
    if (int rc = c->sync_all()) return rc;
    std::lock_guard<std::mutex> lk(c->prof_mu);
    for (auto &r : c->prof_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            if (c->prof_n[r.id] == 0 || ms < c->prof_min[r.id]) c->prof_min[r.id] = ms;
            if (c->prof_n[r.id] == 0 || ms > c->prof_max[r.id]) c->prof_max[r.id] = ms;
            c->prof_ms[r.id] += ms; c->prof_n[r.id] += 1;
        }
        c->prof_pool.push_back(r.a); c->prof_pool.push_back(r.b);
    }
    c->prof_pending.clear();
    return CSDR_OK;
}
extern "C" int csdr_ctx_profile_enable(csdr_ctx *c, int on) {
    DeviceScope dev__(c);
    if (!c) return fail(CSDR_EINVAL, "ctx is null");
    if (int rc = prof_drain(c)) return rc;
    c->prof_on = on != 0;
    c->prof_period = on > 1 ? on : 1;
    if (on) for (int i = 0; i < KID_COUNT; i++) { c->prof_ms[i] = 0.0; c->prof_min[i] = 0.0; c->prof_max[i] = 0.0; c->prof_n[i] = 0; c->prof_seen[i] = 0; }
    return CSDR_OK;
}
extern "C" int csdr_ctx_profile_launches(csdr_ctx *c, int id, int64_t *launches) {
    if (!c || id < 0 || id >= KID_COUNT || !launches) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lk(c->prof_mu);
    *launches = (int64_t)c->prof_seen[id];
    return CSDR_OK;
}
extern "C" int csdr_ctx_profile_range(csdr_ctx *c, int id, double *min_ms, double *max_ms) {
    DeviceScope dev__(c);
    if (!c || id < 0 || id >= KID_COUNT || !min_ms || !max_ms) return fail(CSDR_EINVAL, "bad argument");
    if (int rc = prof_drain(c)) return rc;
    *min_ms = c->prof_n[id] ? c->prof_min[id] : 0.0; *max_ms = c->prof_n[id] ? c->prof_max[id] : 0.0;
    return CSDR_OK;
}
extern "C" int csdr_ctx_profile_num_kernels(void) { return KID_COUNT; }
extern "C" const char *csdr_ctx_profile_kernel_name(int id) { return (id >= 0 && id < KID_COUNT) ? kKernelNames[id] : ""; }
extern "C" int csdr_ctx_profile_fetch(csdr_ctx *c, int id, double *total_ms, int64_t *launches) {
    DeviceScope dev__(c);
    if (!c || id < 0 || id >= KID_COUNT || !total_ms || !launches) return fail(CSDR_EINVAL, "bad argument");
    if (int rc = prof_drain(c)) return rc;
    *total_ms = c->prof_ms[id]; *launches = c->prof_n[id];
    return CSDR_OK;
}

extern "C" int csdr_dev_alloc(csdr_ctx *c, uint64_t bytes, void **dev) {
    DeviceScope dev__(c);
    if (!c || !dev) return fail(CSDR_EINVAL, "null argument");
    if (hipMalloc(dev, bytes) != hipSuccess) return fail(CSDR_ENOMEM, "hipMalloc(%llu) failed", (unsigned long long)bytes);
    return CSDR_OK;
}
extern "C" int csdr_dev_free(csdr_ctx *c, void *dev) {
    DeviceScope dev__(c); (void)c; if (dev) CSDR_HIP_TRY(hipFree(dev)); return CSDR_OK; }
extern "C" int csdr_dev_upload(csdr_ctx *c, void *dev, const void *host, uint64_t bytes) {
    DeviceScope dev__(c);
    if (!c) return fail(CSDR_EINVAL, "ctx is null");
    CSDR_HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    CSDR_HIP_TRY(hipStreamSynchronize(c->stream));
    return CSDR_OK;
}
extern "C" int csdr_dev_download(csdr_ctx *c, void *host, const void *dev, uint64_t bytes) {
    DeviceScope dev__(c);
    if (!c) return fail(CSDR_EINVAL, "ctx is null");
    if (int rc = c->sync_all()) return rc;
    CSDR_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    CSDR_HIP_TRY(hipStreamSynchronize(c->stream));
    return CSDR_OK;
}

extern "C" int csdr_host_register(csdr_ctx *c, void *host, uint64_t bytes) {
    DeviceScope dev__(c);
    if (!c || !host || !bytes) return fail(CSDR_EINVAL, "bad argument");
    CSDR_HIP_TRY(hipHostRegister(host, bytes, hipHostRegisterDefault));
    return CSDR_OK;
}
extern "C" int csdr_host_unregister(csdr_ctx *c, void *host) {
    DeviceScope dev__(c);
    if (!c || !host) return fail(CSDR_EINVAL, "bad argument");
    CSDR_HIP_TRY(hipHostUnregister(host));
    return CSDR_OK;
}

