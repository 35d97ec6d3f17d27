// tests/cpp/test_stream_order.cpp -- cubicsdr_amd/csrc/stream_order.hpp on the host, against a happens-before model of streams and events.
// Built with g++ and -I tests/emu (the HIP types); the handful of HIP functions the header calls are defined HERE, not by the emulation runtime:
// every stream has a tick (work enqueued so far) and a view (the tick of every other stream it is ordered behind); hipEventRecord snapshots the
// stream's view and tick into the event, hipStreamWaitEvent merges the event's snapshot into the waiting stream.  Creates, destroys and
// synchronises are counted and logged; the n-th create fails on request.
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../cubicsdr_amd/csrc/stream_order.hpp"

using namespace csdr;

typedef std::map<const hipEmuStream *, long> View;
struct hipEmuStream { long tick = 0; View seen; };
struct hipEmuEvent { View at; };

static std::set<void *> g_live;              // what was created and not yet destroyed
static std::vector<std::string> g_log;       // create / destroy / synchronise calls in order
static int g_creates = 0, g_fail_create = 0; // the g_fail_create-th create fails (0: none)
static int g_waits = 0, g_records = 0, g_bad = 0;

static bool create_fails() { return ++g_creates == g_fail_create; }
static int count(const char *what) { int n = 0; for (const std::string &s : g_log) n += s == what; return n; }
static void freed(void *p) { if (!g_live.erase(p)) { std::printf("FAIL: %p destroyed twice or never created\n", p); ++g_bad; } }

const char *hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
    if (create_fails()) return hipErrorInvalidValue;
    *s = new hipEmuStream(); g_live.insert(*s); g_log.push_back("stream_create"); return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { freed(s); delete s; g_log.push_back("stream_destroy"); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { g_log.push_back("stream_sync"); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    if (create_fails()) return hipErrorInvalidValue;
    *e = new hipEmuEvent(); g_live.insert(*e); g_log.push_back("event_create"); return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { freed(e); delete e; g_log.push_back("event_destroy"); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { g_log.push_back("event_sync"); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { ++g_records; e->at = s->seen; e->at[s] = s->tick; return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    ++g_waits;
    for (const auto &kv : e->at) if (kv.first != s && s->seen[kv.first] < kv.second) s->seen[kv.first] = kv.second;
    return hipSuccess;
}

static long work(hipEmuStream &s) { return ++s.tick; }                                 // something is enqueued on s
static bool saw(const hipEmuStream &s, const hipEmuStream &of, long tick) {          // s is ordered behind `of` up to `tick`
    auto it = s.seen.find(&of);
    return it != s.seen.end() && it->second >= tick;
}
static bool saw_nothing_of(const hipEmuStream &s, const hipEmuStream &of) { auto it = s.seen.find(&of); return it == s.seen.end() || it->second == 0; }

#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } } while (0)

static void one_reader() {
    hipEmuStream producer, reader, writer;
    ReadGate g;
    const long made = work(producer);
    CHECK(g.acquire(&producer, &reader) == CSDR_OK);
    CHECK(saw(reader, producer, made));
    const long read = work(reader);
    CHECK(g.release(&reader) == CSDR_OK && g.pending);
    CHECK(saw_nothing_of(writer, reader));
    CHECK(g.wait(&writer) == CSDR_OK && !g.pending);
    CHECK(saw(writer, reader, read));
    const int waits = g_waits, records = g_records;
    CHECK(g.wait(&writer) == CSDR_OK);                       // a second wait enqueues nothing
    CHECK(g_waits == waits && g_records == records);
    g.destroy();
}

static void two_readers(bool a_first) {
    hipEmuStream producer, ra, rb, writer;
    ReadGate g;
    work(producer);
    CHECK(g.acquire(&producer, &ra) == CSDR_OK);
    CHECK(g.acquire(&producer, &rb) == CSDR_OK);
    const long read_a = work(ra), read_b = work(rb);
    CHECK(g.release(a_first ? &ra : &rb) == CSDR_OK);
    CHECK(g.release(a_first ? &rb : &ra) == CSDR_OK);
    CHECK(g.wait(&writer) == CSDR_OK);
    CHECK(saw(writer, ra, read_a));                          // the first mark is not lost under the second
    CHECK(saw(writer, rb, read_b));
    g.destroy();
}

static void parities() {
    hipEmuStream producer, r0, r1, writer;
    ReadGate g[2];
    work(producer);
    CHECK(g[0].acquire(&producer, &r0) == CSDR_OK);
    const long read0 = work(r0);
    CHECK(g[0].release(&r0) == CSDR_OK);
    CHECK(!g[1].pending && !g[1].ev_ready && !g[1].ev_read);
    const int waits = g_waits;
    CHECK(g[1].wait(&writer) == CSDR_OK);                    // the other parity's writer is not held up
    CHECK(g_waits == waits && saw_nothing_of(writer, r0) && g[0].pending);
    CHECK(g[1].acquire(&producer, &r1) == CSDR_OK);
    const long read1 = work(r1);
    CHECK(g[1].release(&r1) == CSDR_OK);
    CHECK(g[1].wait(&writer) == CSDR_OK);
    CHECK(saw(writer, r1, read1) && saw_nothing_of(writer, r0) && g[0].pending);
    CHECK(g[0].wait(&writer) == CSDR_OK && saw(writer, r0, read0));
    g[0].destroy(); g[1].destroy();
}

static void never_acquired() {
    hipEmuStream writer;
    g_log.clear();
    ReadGate g;
    CHECK(g.wait(&writer) == CSDR_OK);
    CHECK(g.sync() == CSDR_OK);
    g.destroy();
    CHECK(g_log.empty());                                    // no event was created, synchronised or destroyed
}

static void release_only() {                                 // the block plan's form: readers ordered elsewhere, the mark alone
    hipEmuStream ra, rb, writer;
    ReadGate g;
    const long read_a = work(ra), read_b = work(rb);
    CHECK(g.release(&ra) == CSDR_OK && g.release(&rb) == CSDR_OK);
    CHECK(g.ev_ready == nullptr);
    CHECK(g.wait(&writer) == CSDR_OK && saw(writer, ra, read_a) && saw(writer, rb, read_b));
    g.destroy();
}

static void destroy_pending() {
    hipEmuStream producer, reader;
    ReadGate g;
    CHECK(g.acquire(&producer, &reader) == CSDR_OK && g.release(&reader) == CSDR_OK);
    g_log.clear();
    g.destroy();
    CHECK(count("event_sync") == 1 && count("event_destroy") == 2);
    CHECK(!g_log.empty() && g_log[0] == "event_sync");       // before any destroy
    g.destroy();                                             // and once
    CHECK(count("event_sync") == 1 && count("event_destroy") == 2);
}

static void side_stream() {
    csdr_ctx ctx;
    hipEmuStream boundary, lane, other;
    ctx.stream = &boundary;
    SideStream s;
    g_fail_create = 0;
    CHECK(s.create(&ctx) == CSDR_OK && s.ctx == &ctx && s.st && s.ev_in && s.ev_out);
    const long fed = work(boundary), laned = work(lane);
    work(other);
    CHECK(s.after_boundary() == CSDR_OK);
    CHECK(saw(*s.st, boundary, fed) && saw_nothing_of(*s.st, lane) && saw_nothing_of(*s.st, other));
    CHECK(s.after(&lane) == CSDR_OK);
    CHECK(saw(*s.st, lane, laned) && saw(*s.st, boundary, fed) && saw_nothing_of(*s.st, other));
    CHECK(boundary.seen.empty() && lane.seen.empty() && other.seen.empty());
    const long done = work(*s.st);
    CHECK(s.hand_over() == CSDR_OK);
    CHECK(saw(boundary, *s.st, done) && saw_nothing_of(lane, *s.st) && other.seen.empty());
    g_log.clear();
    s.destroy();
    CHECK(g_log.size() == 4 && g_log[0] == "stream_sync" && count("stream_destroy") == 1 && count("event_destroy") == 2);
    CHECK(g_live.empty());
    // a create that fails at each of its steps: destroy frees what exists, once
    for (int step = 1; step <= 3; ++step) {
        SideStream h;
        g_creates = 0; g_fail_create = step;
        g_log.clear();
        CHECK(h.create(&ctx) == CSDR_EHIP);
        CHECK((int)g_live.size() == step - 1);
        h.destroy();
        CHECK(g_live.empty());
        CHECK(count("stream_destroy") == (step > 1 ? 1 : 0) && count("event_destroy") == (step > 2 ? 1 : 0));
        h.destroy();
        CHECK(count("stream_destroy") == (step > 1 ? 1 : 0) && count("event_destroy") == (step > 2 ? 1 : 0));
    }
    g_fail_create = 0;
}

static void slot_order() {
    SlotOrder o;
    std::vector<int> frames(5, 0);
    const int items[] = {3, 1, 3, 3, 1};                     // the slots of a call's items, in item order
    o.count_begin(5);
    for (int s : items) o.count_job(s);
    CHECK(o.order() == 5);
    CHECK(o.run_slots == std::vector<int>({1, 3}) && o.job_at[1] == 0 && o.job_at[3] == 2);
    std::vector<size_t> at;
    for (int s : items) at.push_back(o.next_job(s));
    CHECK(at == std::vector<size_t>({2, 0, 3, 4, 1}));       // slot by slot, each slot's jobs in item order
    o.rewind();
    CHECK(o.next_job(3) == 2 && o.next_job(1) == 0);
    std::vector<SlotRun> runs(2);
    CHECK(o.run_bytes() == 2 * sizeof(SlotRun));
    o.fill_runs(reinterpret_cast<char *>(runs.data()));
    CHECK(runs[0].slot == 1 && runs[0].job0 == 0 && runs[0].n_jobs == 2 && runs[0].pad == 0);
    CHECK(runs[1].slot == 3 && runs[1].job0 == 2 && runs[1].n_jobs == 3 && runs[1].pad == 0);
    auto commit = [&]() { o.commit([&](int s) { frames[(size_t)s] = 0; }, [&](int s) { frames[(size_t)s] = o.n_jobs_of[(size_t)s]; }); };
    commit();
    CHECK(frames == std::vector<int>({0, 2, 0, 3, 0}));
    o.count_begin(5);
    o.count_job(4); o.count_job(3);
    CHECK(o.order() == 2);
    commit();                                                // the slots of the last call go to zero, the slots of this call take their counts
    CHECK(frames == std::vector<int>({0, 0, 0, 1, 1}) && o.touched == std::vector<int>({3, 4}));
    o.count_begin(5);
    CHECK(o.order() == 0 && o.run_bytes() == 0);
    commit();
    CHECK(frames == std::vector<int>(5, 0) && o.touched.empty());
}

int main() {
    static_assert(sizeof(SlotRun) == 16, "the run record the kernels read");
    one_reader();
    two_readers(true);
    two_readers(false);
    parities();
    never_acquired();
    release_only();
    destroy_pending();
    side_stream();
    slot_order();
    CHECK(g_live.empty());
    if (g_bad) { std::printf("stream order: %d checks failed\n", g_bad); return 1; }
    std::printf("stream order ok\n");
    return 0;
}
