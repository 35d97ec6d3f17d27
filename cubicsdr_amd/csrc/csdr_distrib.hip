// csdr_distrib.hip -- implementation of include/csdr_hip.h (gfx950): csdr_distrib (FFTDataDistributor, src/process/FFTDataDistributor.cpp).
// One csdr_distrib_push is one popped input of FFTDataDistributor::process (:41-143): the buffer bookkeeping and the line pacing are host integer and
// double arithmetic in the reference's order of operations (file:line cited per statement); the samples never come to the host -- distrib_gather
// (kernels_distrib.hpp) copies the emitted lines and the carried partial line inside HBM.  All work of one distributor is enqueued on a stream of
// its own; the spectrum that takes the lines (csdr_spec_process_distrib) is ordered against it by events.
#include <algorithm>
#include <climits>
#include <memory>
#include <vector>

#define CSDR_TU_DISTRIB 1       // this unit is the home of its kernel (kernels_distrib.hpp)
#include "csdr_objects.hpp"
#include "kernels_distrib.hpp"

using namespace csdr;

struct csdr_distrib : SideStream {               // (ev_in: the producer of a device block -- the boundary stream, then the spectrum's FFT lane)
    int max_lines = 0;
    int fft_size = 2048, lps = 30;                     // setFFTSize / setLinesPerSecond: DEFAULT_FFT_SIZE, DEFAULT_WATERFALL_LPS (ctor :11); read at the next push
    // FFTDataDistributor's state
    double accum = 0.0;                                // lineRateAccum
    int64_t rate = 0, freq = 0;                        // inputBuffer.sampleRate / .frequency
    int64_t buffered = 0, offset = 0, buffer_max = 0;  // bufferedItems, bufferOffset, bufferMax
    int64_t dropped = 0;                               // of the last push
    int n_lines = 0, line_len = 0;                     // of the last push
    // the buffered samples (fewer than the largest fft_size so far) in two copies: a push reads one and writes the other
    DevBuf<float2> carry[2];
    int carry_cur = 0;
    // two line batches written alternately, each with the table of its lines' starts (page-locked twin: uploaded per push)
    DevBuf<float2> batch[2];
    DevBuf<int> starts[2];
    PinBuf<int> starts_h[2];
    int cur = 1;                                       // batch of the last push
    hipEvent_t ev_gather[2] = {nullptr, nullptr};      // behind the gather that filled batch k
    bool gathered[2] = {false, false};
    ReadGate read[2];                                  // the spectrum's reads of batch k (csdr_spec_process_distrib); the readers wait for ev_gather
    DevBuf<float2> stage;                              // a host block on its way
};

extern "C" int csdr_distrib_create(csdr_ctx *ctx, int max_lines, csdr_distrib **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    if (max_lines < 1 || max_lines > (1 << 24)) return fail(CSDR_EINVAL, "max_lines %d: 1 .. 2^24", max_lines);
    std::unique_ptr<csdr_distrib, void (*)(csdr_distrib *)> d(new csdr_distrib(), csdr_distrib_destroy);
    d->max_lines = max_lines;
    if (int rc = d->create(ctx)) return rc;
    for (int k = 0; k < 2; ++k) {
        if (int rc = order_event(&d->ev_gather[k])) return rc;
        if (int rc = d->starts[k].reserve((size_t)max_lines)) return rc;
        if (int rc = d->starts_h[k].reserve((size_t)max_lines)) return rc;
    }
    *out = d.release();
    return CSDR_OK;
}

extern "C" void csdr_distrib_destroy(csdr_distrib *d) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d) return;
    for (int k = 0; k < 2; ++k) d->read[k].destroy();                                                  // (a spectrum may still read the batch)
    d->destroy();
    for (int k = 0; k < 2; ++k) {
        if (d->ev_gather[k]) (void)hipEventDestroy(d->ev_gather[k]);
        d->carry[k].release(); d->batch[k].release(); d->starts[k].release(); d->starts_h[k].release();
    }
    d->stage.release();
    delete d;
}

extern "C" int csdr_distrib_set_fft_size(csdr_distrib *d, int n) {                      // setFFTSize :15-18
    if (!d) return fail(CSDR_EINVAL, "distributor is null");
    if (n < 1) return fail(CSDR_EINVAL, "fft_size %d", n);
    d->fft_size = n;
    return CSDR_OK;
}
extern "C" int csdr_distrib_set_lines_per_second(csdr_distrib *d, int lps) {            // setLinesPerSecond :20-22
    if (!d) return fail(CSDR_EINVAL, "distributor is null");
    if (lps < 0) return fail(CSDR_EINVAL, "lines per second %d", lps);
    d->lps = lps;
    return CSDR_OK;
}

// a buffer a kernel in flight may still use is about to be replaced by a larger one
static int distrib_grow(csdr_distrib *d, DevBuf<float2> &b, size_t n, int reader) {
    if (n <= b.cap) return CSDR_OK;
    if (reader >= 0) if (int rc = d->read[reader].sync()) return rc;
    CSDR_HIP_TRY(hipStreamSynchronize(d->st));
    return b.reserve(n);
}

extern "C" int csdr_distrib_push(csdr_distrib *d, const float *iq, int iq_is_dev, int n_samples, int64_t frequency, int64_t sample_rate, int *n_lines_out) {
    RangeScope range__("csdr_distrib_push");
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (n_lines_out) *n_lines_out = 0;
    if (!d) return fail(CSDR_EINVAL, "distributor is null");
    if (sample_rate <= 0 || n_samples < 0 || (n_samples > 0 && !iq)) return fail(CSDR_EINVAL, "bad block arguments (%d samples at %lld S/s)", n_samples, (long long)sample_rate);
    if (iq_is_dev && ((uintptr_t)iq & 7)) return fail(CSDR_EINVAL, "device IQ pointer must be 8-byte aligned");
    // ---- the bookkeeping of one popped input on copies of the state: a refused push leaves everything where it was
    const int64_t fft = d->fft_size;
    const int lps = d->lps;
    double accum = d->accum;
    int64_t buffered = d->buffered, offset = d->offset, buffer_max = d->buffer_max;
    if (d->rate != sample_rate || d->freq != frequency) {                               // :42-53: everything buffered is dropped
        buffer_max = std::max((int64_t)((double)sample_rate * 0.250), (int64_t)(1.2 * (double)fft));      // FFT_DISTRIBUTOR_BUFFER_IN_SECONDS
        offset = 0;
        buffered = 0;
    }
    if (buffer_max < (int64_t)(1.2 * (double)fft)) buffer_max = (int64_t)(1.2 * (double)fft);              // :56-59
    const int64_t carried = buffered;                                                   // V = carry[0 : carried) ++ block[0 : n_add)
    int64_t n_add = n_samples;                                                          // :61
    if (offset + buffered + n_samples > buffer_max) {                                   // :66-76
        offset = 0;
        if (buffered + n_samples > buffer_max) n_add = buffer_max - buffered;
    }
    buffered += n_add;                                                                  // :80
    if (buffered > INT_MAX) return fail(CSDR_ERANGE, "%lld buffered samples", (long long)buffered);
    const double inputTime = (double)buffered / (double)sample_rate;                    // :89
    const double inputLines = (double)buffered / (double)fft;                           // :91
    const double lineRateStep = ((double)lps * inputTime) / (double)inputLines;         // :96
    const int k = d->cur ^ 1;                                                           // the batch this push fills
    // (the table of batch k is page-locked memory the upload of two pushes ago read: that upload lies in front of its gather)
    if (d->gathered[k]) CSDR_HIP_TRY(hipEventSynchronize(d->ev_gather[k]));
    int *starts = d->starts_h[k].p;
    int n_lines = 0;
    int64_t processed = 0;
    if (buffered >= fft) {                                                              // :99
        if (accum + (lineRateStep * ((double)buffered / (double)fft)) < 1.0) {          // :101-104: move along
            accum += (lineRateStep * ((double)buffered / (double)fft));
            processed = buffered;
        } else {
            for (int64_t i = 0, iMax = buffered; i < iMax; i += fft) {                  // :106-129
                if ((i + fft) > iMax) break;
                accum += lineRateStep;
                if (accum >= 1.0) {
                    if (n_lines == d->max_lines) return fail(CSDR_ERANGE, "the push emits more than max_lines %d lines", d->max_lines);
                    starts[n_lines++] = (int)i;
                    while (accum >= 1.0) accum -= 1.0;
                }
                processed += fft;
            }
        }
    }
    const int64_t tail = buffered - processed;
    // ---- the samples: lines into batch k, the unconsumed tail into the other carry
    const int out_c = d->carry_cur ^ 1;
    if (int rc = distrib_grow(d, d->carry[out_c], (size_t)std::max<int64_t>(tail, 1), -1)) return rc;
    if (int rc = distrib_grow(d, d->batch[k], (size_t)std::max<int64_t>((int64_t)n_lines * fft, 1), k)) return rc;
    if (n_lines > 0 || tail > 0) {
        csdr_ctx *c = d->ctx;
        const float2 *block = (const float2 *)iq;
        if (n_add > 0 && iq_is_dev) {
            // the block's producer: work on the boundary stream (the rule of csdr_spec_process for a device input) and, for a block of the ingest,
            // the transfer every stream of the context was made to wait for -- the spectrum's FFT lane stands for them
            if (!(c->own_stream && !c->boundary_shared)) if (int rc = d->after_boundary()) return rc;
            if (int rc = d->after(c->lanes[LANE_FFT])) return rc;
        } else if (n_add > 0) {
            if (int rc = distrib_grow(d, d->stage, (size_t)n_add, -1)) return rc;
            CSDR_HIP_TRY(hipMemcpyAsync(d->stage.p, iq, (size_t)n_add * sizeof(float2), hipMemcpyHostToDevice, d->st));
            block = d->stage.p;
        }
        if (n_lines > 0) CSDR_HIP_TRY(hipMemcpyAsync(d->starts[k].p, starts, (size_t)n_lines * sizeof(int), hipMemcpyHostToDevice, d->st));
        if (int rc = d->read[k].wait(d->st)) return rc;                                 // the spectrum's reads of the batch being rewritten
        DistribArgs a{};
        a.carry_in = d->carry[d->carry_cur].p; a.block = block; a.lines = d->batch[k].p; a.carry_out = d->carry[out_c].p;
        a.starts = d->starts[k].p;
        a.buffered = (int)carried; a.fft = (int)fft; a.n_lines = n_lines;
        a.tail_start = (int)processed; a.tail_len = (int)tail;
        const int64_t longest = std::max<int64_t>(n_lines > 0 ? fft : 0, tail);
        const int64_t pieces = (longest + 2) / 2;
        const dim3 grid((unsigned)((pieces + kDgThreads * kDgPieces - 1) / (kDgThreads * kDgPieces)), (unsigned)std::min(n_lines + 1, 65535));
        { ProfScope ps__(c, KID_DISTRIB_GATHER, d->st); hipLaunchKernelGGL(distrib_gather, grid, dim3(kDgThreads), 0, d->st, a); }
        CSDR_HIP_TRY(hipGetLastError());
        CSDR_HIP_TRY(hipEventRecord(d->ev_gather[k], d->st));
        d->gathered[k] = true;
        // whoever recycles a device block orders itself behind the context's streams (the ingest's ring): the gather's reads join the FFT lane
        if (n_add > 0 && iq_is_dev) CSDR_HIP_TRY(hipStreamWaitEvent(c->lanes[LANE_FFT], d->ev_gather[k], 0));
    }
    // ---- commit
    d->rate = sample_rate; d->freq = frequency;
    d->accum = accum; d->buffer_max = buffer_max;
    d->dropped = (int64_t)n_samples - n_add;
    if (processed) { buffered -= processed; offset += processed; }                      // :133-136
    if (buffered <= 0) { buffered = 0; offset = 0; }                                    // :138-141
    d->buffered = buffered; d->offset = offset;
    d->carry_cur = out_c;
    d->cur = k; d->n_lines = n_lines; d->line_len = (int)fft;
    if (n_lines_out) *n_lines_out = n_lines;
    return CSDR_OK;
}

extern "C" int csdr_distrib_get_state(const csdr_distrib *d, csdr_distrib_state *st) {
    if (!d || !st) return fail(CSDR_EINVAL, "null argument");
    st->line_rate_accum = d->accum;
    st->buffered_items = d->buffered; st->buffer_offset = d->offset; st->buffer_max = d->buffer_max; st->dropped = d->dropped;
    st->n_lines = d->n_lines; st->line_len = d->line_len;
    return CSDR_OK;
}

extern "C" int csdr_distrib_lines(csdr_distrib *d, const float **dev_lines, int *n_lines, int *line_len) {
    if (!d || !dev_lines || !n_lines || !line_len) return fail(CSDR_EINVAL, "null argument");
    *dev_lines = (const float *)d->batch[d->cur].p; *n_lines = d->n_lines; *line_len = d->line_len;
    return CSDR_OK;
}

extern "C" int csdr_distrib_fetch_lines(csdr_distrib *d, float *host, int64_t cap_floats, int *n_lines) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !n_lines) return fail(CSDR_EINVAL, "null argument");
    *n_lines = 0;
    const int64_t need = 2 * (int64_t)d->n_lines * d->line_len;
    if (need > 0 && !host) return fail(CSDR_EINVAL, "host buffer is null");
    if (cap_floats < need) return fail(CSDR_ERANGE, "need %lld floats", (long long)need);
    if (need > 0) CSDR_HIP_TRY(hipMemcpyAsync(host, d->batch[d->cur].p, (size_t)need * sizeof(float), hipMemcpyDeviceToHost, d->st));
    CSDR_HIP_TRY(hipStreamSynchronize(d->st));
    *n_lines = d->n_lines;
    return CSDR_OK;
}

extern "C" int csdr_distrib_fetch_buffered(csdr_distrib *d, float *host, int64_t cap_floats, int *n) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!d || !n) return fail(CSDR_EINVAL, "null argument");
    *n = 0;
    const int64_t need = 2 * d->buffered;
    if (need > 0 && !host) return fail(CSDR_EINVAL, "host buffer is null");
    if (cap_floats < need) return fail(CSDR_ERANGE, "need %lld floats", (long long)need);
    if (need > 0) CSDR_HIP_TRY(hipMemcpyAsync(host, d->carry[d->carry_cur].p, (size_t)need * sizeof(float), hipMemcpyDeviceToHost, d->st));
    CSDR_HIP_TRY(hipStreamSynchronize(d->st));
    *n = (int)d->buffered;
    return CSDR_OK;
}

// The lines of the last push as process() inputs, in order (what FFTVisualDataThread's queue between the distributor and the processor carries,
// FFTVisualDataThread.cpp:58-70): read where the gather put them.
extern "C" int csdr_spec_process_distrib(csdr_spec *spec, csdr_distrib *d) {
    DeviceScope dev__(d ? d->ctx : nullptr);
    if (!spec || !d) return fail(CSDR_EINVAL, "null argument");
    csdr_ctx *c = d->ctx;
    if (spec_ctx(spec) != c) return fail(CSDR_EINVAL, "the spectrum belongs to another context");
    const int n = d->n_lines, len = d->line_len, k = d->cur;
    if (n == 0) return CSDR_OK;
    const int want = csdr_spec_desired_input_size(spec);
    if (want <= 0) return fail(CSDR_ESTATE, "spec not set up");
    const bool view = csdr_spec_get_view(spec) != 0;
    // the spectrum's lanes wait for the gather (a zoomed view reads its input on the channelizer's lane)
    CSDR_HIP_TRY(hipStreamWaitEvent(c->lanes[LANE_FFT], d->ev_gather[k], 0));
    if (view && !c->same(LANE_POST, LANE_FFT)) CSDR_HIP_TRY(hipStreamWaitEvent(c->lanes[LANE_POST], d->ev_gather[k], 0));
    const float *lines = (const float *)d->batch[k].p;
    int rc = CSDR_OK;
    if (view) {                                         // every call is one input
        for (int l = 0; l < n && rc == CSDR_OK; ++l) rc = csdr_spec_process(spec, lines + 2 * (size_t)l * len, 1, 1, len, CSDR_SPEC_FIRST_FRAME);
    } else rc = csdr_spec_process(spec, lines, 1, n, len, len >= want ? CSDR_SPEC_FIRST_FRAME : CSDR_SPEC_LINES);
    // the distributor rewrites this batch at its second push from here: behind these reads (also those of a call that failed half-way)
    if (int rc2 = d->read[k].release(c->lanes[LANE_FFT])) return rc2;
    return rc;
}
