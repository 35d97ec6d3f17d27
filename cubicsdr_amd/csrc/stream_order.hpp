// stream_order.hpp -- how the objects behind include/csdr_hip.h order themselves against each other on the device, stated once:
// ReadGate, the hand-off of one buffer to readers that stay in HBM; SideStream, an object's own stream beside the context's boundary stream;
// SlotOrder, the slot order of a call whose workgroups each walk one slot's jobs.  Host code only, on top of common.hpp alone.
#pragma once
#include "common.hpp"

namespace csdr {

// an event that only orders streams
inline int order_event(hipEvent_t *ev) {
    CSDR_HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    return CSDR_OK;
}
// `waiter` runs behind everything enqueued on `producer` so far
inline int order_behind(hipEvent_t ev, hipStream_t producer, hipStream_t waiter) {
    CSDR_HIP_TRY(hipEventRecord(ev, producer));
    CSDR_HIP_TRY(hipStreamWaitEvent(waiter, ev, 0));
    return CSDR_OK;
}

// One buffer handed to device-side readers.  acquire: the reader's stream waits for what the producer's stream has enqueued.  release, behind the
// reader's enqueued reads: leaves ONE mark that stands for every reader since the last wait -- a reader that finds a mark pending first waits for
// it, so that the mark it leaves covers both.  wait: whoever rewrites the buffer comes behind that mark.  Nothing here blocks the host but
// sync() and destroy().  The events are created at first use: a gate nobody passes never has them, and a buffer whose readers are ordered by
// another gate's acquire (the bank's block plan) uses release and wait alone.
struct ReadGate {
    hipEvent_t ev_ready = nullptr, ev_read = nullptr;
    bool pending = false;                    // ev_read is recorded and not yet waited for
    int acquire(hipStream_t producer, hipStream_t reader) {
        if (!ev_ready) if (int rc = order_event(&ev_ready)) return rc;
        return order_behind(ev_ready, producer, reader);
    }
    int release(hipStream_t reader) {
        if (!ev_read) if (int rc = order_event(&ev_read)) return rc;
        if (pending) CSDR_HIP_TRY(hipStreamWaitEvent(reader, ev_read, 0));
        CSDR_HIP_TRY(hipEventRecord(ev_read, reader));
        pending = true;
        return CSDR_OK;
    }
    int wait(hipStream_t writer) {           // (one untaken test while nobody reads this way)
        if (!pending) return CSDR_OK;
        CSDR_HIP_TRY(hipStreamWaitEvent(writer, ev_read, 0));
        pending = false;
        return CSDR_OK;
    }
    int sync() {                             // the host waits for the readers: the buffer is about to be freed or replaced
        if (!pending) return CSDR_OK;
        CSDR_HIP_TRY(hipEventSynchronize(ev_read));
        pending = false;
        return CSDR_OK;
    }
    void destroy() {
        (void)sync();
        if (ev_ready) (void)hipEventDestroy(ev_ready);
        if (ev_read) (void)hipEventDestroy(ev_read);
        ev_ready = ev_read = nullptr;
    }
};

// A non-blocking stream of an object's own, on which all of its work runs, with the two events that tie it to the streams around it.  Every
// object that has one is created into a holder whose deleter is the object's destroy, and destroy() takes the object at any stage of create.
struct SideStream {
    csdr_ctx *ctx = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    int create(csdr_ctx *c) {
        ctx = c;
        CSDR_HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        if (int rc = order_event(&ev_in)) return rc;
        return order_event(&ev_out);
    }
    void destroy() {
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_out) (void)hipEventDestroy(ev_out);
        st = nullptr; ev_in = ev_out = nullptr;
    }
    // what `producer` has enqueued (a device input of this call) precedes the work enqueued on st next
    int after(hipStream_t producer) { return order_behind(ev_in, producer, st); }
    int after_boundary() { return after(ctx->stream); }
    // whatever the caller enqueues on the boundary stream next reads what st has finished
    int hand_over() { return order_behind(ev_out, st, ctx->stream); }
};

// The slot order of a call: a workgroup walks one slot's jobs, so the jobs lie slot by slot, each slot's in item order, and one run record per
// slot that has jobs says where.  The caller counts (count_begin, count_job), orders, then walks its items again and takes next_job(slot).
struct SlotRun { int32_t slot, job0, n_jobs, pad; };     // one workgroup: jobs [job0, job0 + n_jobs) of `slot`
struct SlotOrder {
    std::vector<int> n_jobs_of, job_at, cursor, run_slots;     // per slot: jobs of the call, its first job, the next one to fill; the slots that have jobs
    std::vector<int> touched;                                  // the slots of the last committed call
    void count_begin(int max_slots) { n_jobs_of.assign((size_t)max_slots, 0); }
    void count_job(int slot) { ++n_jobs_of[(size_t)slot]; }
    size_t order() {                                           // the jobs of the call
        run_slots.clear();
        job_at.assign(n_jobs_of.size(), 0);
        int at = 0;
        for (int s = 0; s < (int)n_jobs_of.size(); ++s)
            if (n_jobs_of[(size_t)s]) { run_slots.push_back(s); job_at[(size_t)s] = at; at += n_jobs_of[(size_t)s]; }
        cursor = job_at;
        return (size_t)at;
    }
    void rewind() { cursor = job_at; }                         // the items are walked once more
    size_t next_job(int slot) { return (size_t)cursor[(size_t)slot]++; }
    size_t run_bytes() const { return run_slots.size() * sizeof(SlotRun); }
    void fill_runs(char *staging) const {                      // the head of the call's staging set
        SlotRun *runs_h = reinterpret_cast<SlotRun *>(staging);
        for (size_t r = 0; r < run_slots.size(); ++r) {
            const int s = run_slots[r];
            runs_h[r] = SlotRun{s, job_at[(size_t)s], n_jobs_of[(size_t)s], 0};
        }
    }
    // the planned call becomes the state: the slots of the last call go to zero, the slots of this call take their counts
    template <typename Zero, typename Take>
    void commit(Zero &&zero, Take &&take) {
        for (int s : touched) zero(s);
        touched = run_slots;
        for (int s : run_slots) take(s);
    }
};

}  // namespace csdr
