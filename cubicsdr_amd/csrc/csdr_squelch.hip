// csdr_squelch.hip -- implementation of include/csdr_hip.h (gfx950): csdr_squelch, the level / floor / ceiling trackers and the squelch of N
// demodulators whose state and items stay in HBM.  The host plans a call -- one SquelchRun per stepped slot with the settings in force, behind them
// the blocks and the host audio of the explicit form -- and uploads the plan from page-locked staging sets in rotation; ONE launch of squelch_scan
// steps every slot through every block, and where a slot has audio squelch_pack and squelch_pcm16 (kernels_squelch.hpp) write the recorder's packed
// stream.  All work runs on a stream of the object's own, as the scope bank's does; the demodulator bank's sums, audio and block plan are reached
// through bank_audio_acquire / _release and bank_plan_release (csdr_objects.hpp), ordered by events.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#define CSDR_TU_SQUELCH 1     // this unit is the home of its kernels (kernels_squelch.hpp)
#include "csdr_objects.hpp"
#include "kernels_squelch.hpp"

using namespace csdr;

namespace {
constexpr int kSqStage = 2;                  // page-locked staging sets of the plan
struct SqSettings { bool enabled = false, muted = false; int record = CSDR_RECORD_SILENCE; float level_db = 0.0f; };     // squelchEnabled, muted, the sink's option, squelchLevel
}  // namespace

struct csdr_squelch : SideStream {                     // (ev_in: device audio of the caller; ev_out: csdr_squelch_device_items)
    int max_slots = 0, max_blocks = 0;
    std::vector<SqSettings> set;
    std::vector<int> blocks;                           // per slot: blocks stepped by the last process
    std::vector<int> touched;                          // slots the last process stepped
    DevBuf<SquelchState> state;
    DevBuf<csdr_squelch_item> items;
    DevBuf<uint8_t> flags;
    DevBuf<SquelchRec> recs;
    DevBuf<int32_t> totals;
    DevBuf<int64_t> pack;
    DevBuf<int16_t> pcm;
    PinBuf<SquelchState> fresh;                        // one slot as the constructor leaves it: the source of reset_slot's copy
    StageRing<kSqStage> plan;                          // SquelchRun [runs] | csdr_squelch_block [blocks] | float [host audio] of the call being run
    bool recorded = false;                             // the last process wrote a recorder stream
    std::vector<uint8_t> flags_h;                      // the flags of the last process on the host (csdr_squelch_fetch_flags, csdr_mix_push_squelched)
    bool flags_valid = false;
    const csdr_bank *src_bank = nullptr;               // the last process was process_bank of this bank's execute number src_exec
    uint64_t src_exec = 0;
    // scratch of a call's planning
    std::vector<SquelchRun> runs_h;
    std::vector<char> seen;
};

extern "C" int csdr_squelch_create(csdr_ctx *ctx, int max_slots, int max_blocks, csdr_squelch **out) {
    DeviceScope dev__(ctx);
    if (!ctx || !out) return fail(CSDR_EINVAL, "null argument");
    if (max_slots < 1 || max_slots > kSqMaxSlots) return fail(CSDR_EINVAL, "max_slots %d: 1 .. %d", max_slots, kSqMaxSlots);
    if (max_blocks < 1) return fail(CSDR_EINVAL, "max_blocks %d", max_blocks);
    std::unique_ptr<csdr_squelch, void (*)(csdr_squelch *)> sq(new csdr_squelch(), csdr_squelch_destroy);
    sq->max_slots = max_slots; sq->max_blocks = max_blocks;
    if (int rc = sq->create(ctx)) return rc;
    if (int rc = sq->plan.create()) return rc;
    const size_t S = (size_t)max_slots, SB = S * (size_t)max_blocks;
    if (int rc = sq->state.reserve(S)) return rc;
    if (int rc = sq->items.reserve(SB)) return rc;
    if (int rc = sq->flags.reserve(SB)) return rc;
    if (int rc = sq->recs.reserve(SB)) return rc;
    if (int rc = sq->totals.reserve(S)) return rc;
    if (int rc = sq->pack.reserve(S + 1)) return rc;
    if (int rc = sq->fresh.reserve(1)) return rc;
    sq->fresh.p[0] = SquelchState{-100.0f, -30.0f, 30.0f, 0};                           // DemodulatorThread ctor (:20-27)
    std::vector<SquelchState> all(S, sq->fresh.p[0]);
    CSDR_HIP_TRY(hipMemcpy(sq->state.p, all.data(), S * sizeof(SquelchState), hipMemcpyHostToDevice));
    CSDR_HIP_TRY(hipMemset(sq->flags.p, 0, SB));
    sq->set.assign(S, SqSettings{});
    sq->blocks.assign(S, 0);
    sq->flags_h.assign(SB, 0);
    *out = sq.release();
    return CSDR_OK;
}

extern "C" void csdr_squelch_destroy(csdr_squelch *sq) {
    DeviceScope dev__(sq ? sq->ctx : nullptr);
    if (!sq) return;
    sq->destroy();
    sq->plan.destroy();
    sq->state.release(); sq->items.release(); sq->flags.release(); sq->recs.release(); sq->totals.release(); sq->pack.release(); sq->pcm.release();
    sq->fresh.release();
    delete sq;
}

// setSquelchEnabled / setSquelchLevel (DemodulatorThread.cpp:384-397), setMuted (:339-345), the sink's squelch option (AudioSinkFileThread.cpp:19-25):
// read by the next process call
extern "C" int csdr_squelch_set_slot(csdr_squelch *sq, int slot, int enabled, float level_db, int muted, int record_option) {
    if (!sq) return fail(CSDR_ESTATE, "squelch bank is null");
    if (slot < 0 || slot >= sq->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, sq->max_slots);
    if (record_option < CSDR_RECORD_SILENCE || record_option > CSDR_RECORD_ALWAYS) return fail(CSDR_EINVAL, "record option %d: 0 .. 2", record_option);
    SqSettings &s = sq->set[(size_t)slot];
    s.enabled = enabled != 0; s.level_db = level_db; s.muted = muted != 0; s.record = record_option;
    return CSDR_OK;
}

extern "C" int csdr_squelch_reset_slot(csdr_squelch *sq, int slot) {
    DeviceScope dev__(sq ? sq->ctx : nullptr);
    if (!sq) return fail(CSDR_ESTATE, "squelch bank is null");
    if (slot < 0 || slot >= sq->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, sq->max_slots);
    CSDR_HIP_TRY(hipMemcpyAsync(sq->state.p + slot, sq->fresh.p, sizeof(SquelchState), hipMemcpyHostToDevice, sq->st));
    return CSDR_OK;
}

extern "C" int csdr_squelch_get_state(csdr_squelch *sq, int slot, float *level, float *floor, float *ceil, int *squelch_break) {
    DeviceScope dev__(sq ? sq->ctx : nullptr);
    if (!sq) return fail(CSDR_ESTATE, "squelch bank is null");
    if (slot < 0 || slot >= sq->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, sq->max_slots);
    SquelchState s;
    CSDR_HIP_TRY(hipMemcpyAsync(&s, sq->state.p + slot, sizeof s, hipMemcpyDeviceToHost, sq->st));
    CSDR_HIP_TRY(hipStreamSynchronize(sq->st));
    if (level) *level = s.level;
    if (floor) *floor = s.floor;
    if (ceil) *ceil = s.ceil;
    if (squelch_break) *squelch_break = s.brk;
    return CSDR_OK;
}

// The plan and the launches of one call; sq->runs_h passed the caller's checks and holds, per stepped slot, everything but the pointers into the plan.
// in: the explicit form's inputs in the order of runs_h (nullptr: the bank form, whose pointers are final); bank: acquired here, where the call can
// no longer be refused, released behind the kernels.  rec_cap: the samples the recorder can write at most.
static int sq_run(csdr_squelch *sq, const csdr_squelch_input *const *in, csdr_bank *bank, int64_t rec_cap) {
    std::vector<SquelchRun> &runs = sq->runs_h;
    const size_t n_runs = runs.size();
    size_t n_blocks = 0, host_floats = 0;
    int max_nb = 0, max_n_audio = 1;
    bool any_audio = false, any_dev = false;
    for (size_t r = 0; r < n_runs; ++r) {
        max_nb = std::max(max_nb, runs[r].n_blocks);
        any_audio = any_audio || runs[r].audio != nullptr;
        if (!in) continue;
        n_blocks += (size_t)runs[r].n_blocks;
        int64_t a = 0;
        for (int b = 0; b < runs[r].n_blocks; ++b) { a += in[r]->blocks[b].n_audio; max_n_audio = std::max(max_n_audio, in[r]->blocks[b].n_audio); }
        if (in[r]->audio && in[r]->audio_is_dev) any_dev = true;
        else if (in[r]->audio) host_floats += (size_t)a;
    }
    if (bank)
        for (size_t r = 0; r < n_runs; ++r)
            for (const csdr_block_result &br : bank->slots[(size_t)runs[r].slot].results) max_n_audio = std::max(max_n_audio, br.n_audio);
    any_audio = any_audio && rec_cap > 0;
    if (any_audio && (size_t)rec_cap > sq->pcm.cap) {                                  // (a kernel may still write the buffer being replaced)
        CSDR_HIP_TRY(hipStreamSynchronize(sq->st));
        if (int rc = sq->pcm.reserve((size_t)rec_cap)) return rc;
    }
    // ---- commit the host state; from here on the call is enqueued
    for (int s : sq->touched) sq->blocks[(size_t)s] = 0;
    sq->touched.clear();
    for (const SquelchRun &r : runs) { sq->touched.push_back(r.slot); sq->blocks[(size_t)r.slot] = r.n_blocks; }
    sq->flags_valid = false;
    sq->recorded = any_audio;
    sq->src_bank = bank; sq->src_exec = bank ? bank->n_exec : 0;
    const size_t S = (size_t)sq->max_slots;
    CSDR_HIP_TRY(hipMemsetAsync(sq->flags.p, 0, S * (size_t)sq->max_blocks, sq->st));  // the rows of the slots this call does not step
    CSDR_HIP_TRY(hipMemsetAsync(sq->totals.p, 0, S * sizeof(int32_t), sq->st));
    if (n_runs == 0) return CSDR_OK;
    if (bank) { if (int rc = bank_audio_acquire(bank, sq->st)) return rc; }
    else if (any_dev) { if (int rc = sq->after_boundary()) return rc; }
    const size_t off_blocks = n_runs * sizeof(SquelchRun), off_audio = off_blocks + n_blocks * sizeof(csdr_squelch_block);
    const size_t bytes = off_audio + host_floats * sizeof(float);
    if (int rc = sq->plan.begin(sq->st, bytes)) return rc;                             // the one host wait of a call
    if (in) {
        csdr_squelch_block *blocks_h = reinterpret_cast<csdr_squelch_block *>(sq->plan.host() + off_blocks);
        const csdr_squelch_block *blocks_d = reinterpret_cast<const csdr_squelch_block *>(sq->plan.device() + off_blocks);
        float *audio_h = reinterpret_cast<float *>(sq->plan.host() + off_audio);
        const float *audio_d = reinterpret_cast<const float *>(sq->plan.device() + off_audio);
        size_t at_b = 0, at_a = 0;
        for (size_t r = 0; r < n_runs; ++r) {
            const csdr_squelch_input &i = *in[r];
            if (i.n_blocks) memcpy(blocks_h + at_b, i.blocks, (size_t)i.n_blocks * sizeof(csdr_squelch_block));
            runs[r].blocks = blocks_d + at_b;
            at_b += (size_t)i.n_blocks;
            if (i.audio && !i.audio_is_dev) {                                          // host audio rides behind the plan
                size_t a = 0;
                for (int b = 0; b < i.n_blocks; ++b) a += (size_t)i.blocks[b].n_audio;
                if (a) memcpy(audio_h + at_a, i.audio, a * sizeof(float));
                runs[r].audio = audio_d + at_a;
                at_a += a;
            }
        }
    }
    memcpy(sq->plan.host(), runs.data(), n_runs * sizeof(SquelchRun));
    if (int rc = sq->plan.uploaded(sq->st, bytes)) return rc;
    SquelchArgs a{};
    a.runs = reinterpret_cast<const SquelchRun *>(sq->plan.device());
    a.n_runs = (int)n_runs; a.max_blocks = sq->max_blocks;
    a.state = sq->state.p; a.items = sq->items.p; a.flags = sq->flags.p; a.recs = sq->recs.p; a.totals = sq->totals.p; a.pack = sq->pack.p; a.pcm = sq->pcm.p;
    {
        ProfScope ps__(sq->ctx, KID_SQUELCH_SCAN, sq->st);
        hipLaunchKernelGGL(squelch_scan, dim3((unsigned)((n_runs + kSqWaves - 1) / kSqWaves)), dim3(kSqWaves * 64), kSqWaves * sizeof(SquelchLds), sq->st, a);
    }
    if (any_audio) {
        {
            ProfScope ps__(sq->ctx, KID_SQUELCH_PACK, sq->st);
            hipLaunchKernelGGL(squelch_pack, dim3(1), dim3(256), 256 * sizeof(int64_t), sq->st, sq->totals.p, sq->pack.p, sq->max_slots);
        }
        ProfScope ps__(sq->ctx, KID_SQUELCH_PCM16, sq->st);
        hipLaunchKernelGGL(squelch_pcm16, dim3((unsigned)std::max(1, std::min(16, (max_n_audio + 255) / 256)), (unsigned)max_nb, (unsigned)n_runs), dim3(256), 0, sq->st, a);
    }
    CSDR_HIP_TRY(hipGetLastError());
    if (!bank) return CSDR_OK;
    if (int rc = bank_audio_release(bank, sq->st)) return rc;
    return bank_plan_release(bank, sq->st);
}

extern "C" int csdr_squelch_process(csdr_squelch *sq, const csdr_squelch_input *in, int n) {
    DeviceScope dev__(sq ? sq->ctx : nullptr);
    if (!sq) return fail(CSDR_ESTATE, "squelch bank is null");
    if (n < 0 || (n > 0 && !in)) return fail(CSDR_EINVAL, "bad inputs");
    // every check of a call, in front of anything that is enqueued or changed: the whole call is refused or none of it
    sq->seen.assign((size_t)sq->max_slots, 0);
    int64_t rec_cap = 0;
    for (int i = 0; i < n; ++i) {
        const csdr_squelch_input &x = in[i];
        if (x.slot < 0 || x.slot >= sq->max_slots) return fail(CSDR_EINVAL, "input %d: slot %d of %d", i, x.slot, sq->max_slots);
        if (sq->seen[(size_t)x.slot]) return fail(CSDR_EINVAL, "input %d: slot %d twice in one process", i, x.slot);
        sq->seen[(size_t)x.slot] = 1;
        if (x.n_blocks < 0 || x.n_blocks > sq->max_blocks) return fail(CSDR_EINVAL, "input %d: %d blocks, max_blocks %d", i, x.n_blocks, sq->max_blocks);
        if (x.n_blocks > 0 && !x.blocks) return fail(CSDR_EINVAL, "input %d: no blocks", i);
        int64_t a = 0;
        for (int b = 0; b < x.n_blocks; ++b) {
            if (x.blocks[b].n_audio < 0 || x.blocks[b].n_in < 0) return fail(CSDR_EINVAL, "input %d, block %d: negative count", i, b);
            a += x.blocks[b].n_audio;
        }
        if (a > INT32_MAX) return fail(CSDR_EINVAL, "input %d: %lld floats of audio in one call", i, (long long)a);
        if (x.audio) rec_cap += a;
    }
    // the runs in slot order (the recorder's stream is packed in slot order whatever the order of the inputs)
    std::vector<const csdr_squelch_input *> order;
    for (int i = 0; i < n; ++i) if (in[i].n_blocks > 0) order.push_back(in + i);
    std::sort(order.begin(), order.end(), [](const csdr_squelch_input *a, const csdr_squelch_input *b) { return a->slot < b->slot; });
    sq->runs_h.clear();
    for (const csdr_squelch_input *x : order) {
        const SqSettings &s = sq->set[(size_t)x->slot];
        SquelchRun r{};
        r.slot = x->slot; r.n_blocks = x->n_blocks;
        r.enabled = s.enabled; r.muted = s.muted; r.record = s.record; r.level_db = s.level_db;
        r.sample_rate = x->sample_rate; r.ash = 0;
        r.audio = x->audio;                                                             // (host audio: replaced by its place behind the plan)
        sq->runs_h.push_back(r);
    }
    return sq_run(sq, order.data(), nullptr, rec_cap);
}

extern "C" int csdr_squelch_process_bank(csdr_squelch *sq, csdr_bank *bank) {
    DeviceScope dev__(sq ? sq->ctx : nullptr);
    if (!sq) return fail(CSDR_ESTATE, "squelch bank is null");
    if (!bank) return fail(CSDR_EINVAL, "bank is null");
    if (bank->ctx != sq->ctx) return fail(CSDR_EINVAL, "the bank belongs to another context");
    if (bank->last_nb == 0) return fail(CSDR_ESTATE, "no csdr_bank_execute yet");
    if (bank->last_nb > sq->max_blocks) return fail(CSDR_EINVAL, "the execute had %d blocks, max_blocks %d", bank->last_nb, sq->max_blocks);
    // one run for every slot DemodulatorThread::run would have seen blocks of: configured and active, routed (it has results), pushed (not skipped by
    // the shift rule), with a modem of the library's own (a front-end-only or host slot forms no level here)
    sq->runs_h.clear();
    int64_t rec_cap = 0;
    const int ns = std::min(sq->max_slots, bank->max_demods), NB = bank->last_nb;
    for (int si = 0; si < ns; ++si) {
        const SlotHost &s = bank->slots[(size_t)si];
        if (!s.configured || !s.active || s.results.empty() || s.results[0].skipped) continue;
        if (s.prm.modem == CSDR_MODEM_HOST || s.prm.modem == CSDR_MODEM_FRONTEND_ONLY) continue;
        const SqSettings &q = sq->set[(size_t)si];
        SquelchRun r{};
        r.slot = si; r.n_blocks = (int)s.results.size();
        r.enabled = q.enabled; r.muted = q.muted; r.record = q.record; r.level_db = q.level_db;
        r.sample_rate = s.prm.bandwidth;                                                // sampleTime = n_iq / bandwidth (host/HipPipeline.h)
        r.ash = s.last_ash;
        r.bout = s.cfg.bout;
        r.plan = bank_last_plans(bank) + (size_t)si * (size_t)(NB + 1);
        r.audio = s.last_ash < 0 ? nullptr : s.cfg.audio;
        rec_cap += s.last_A;
        sq->runs_h.push_back(r);
    }
    return sq_run(sq, nullptr, bank, rec_cap);
}

extern "C" int csdr_squelch_blocks(const csdr_squelch *sq, int slot) {
    return sq && slot >= 0 && slot < sq->max_slots ? sq->blocks[(size_t)slot] : 0;
}

extern "C" int csdr_squelch_fetch(csdr_squelch *sq, int slot, csdr_squelch_item *out, int cap, int *n) {
    DeviceScope dev__(sq ? sq->ctx : nullptr);
    if (!sq) return fail(CSDR_ESTATE, "squelch bank is null");
    if (!out || !n) return fail(CSDR_EINVAL, "null argument");
    if (slot < 0 || slot >= sq->max_slots) return fail(CSDR_EINVAL, "slot %d of %d", slot, sq->max_slots);
    const int nb = sq->blocks[(size_t)slot];
    if (nb > cap) return fail(CSDR_ERANGE, "need room for %d items", nb);
    *n = nb;
    if (!nb) return CSDR_OK;
    CSDR_HIP_TRY(hipMemcpyAsync(out, sq->items.p + (size_t)slot * (size_t)sq->max_blocks, (size_t)nb * sizeof(csdr_squelch_item), hipMemcpyDeviceToHost, sq->st));
    CSDR_HIP_TRY(hipStreamSynchronize(sq->st));
    return CSDR_OK;
}

// the flags of the last process on the host: ONE copy for the whole bank, kept until the next process
static int sq_flags(csdr_squelch *sq) {
    if (sq->flags_valid) return CSDR_OK;
    CSDR_HIP_TRY(hipMemcpyAsync(sq->flags_h.data(), sq->flags.p, sq->flags_h.size(), hipMemcpyDeviceToHost, sq->st));
    CSDR_HIP_TRY(hipStreamSynchronize(sq->st));
    sq->flags_valid = true;
    return CSDR_OK;
}

extern "C" int csdr_squelch_fetch_flags(csdr_squelch *sq, uint8_t *out, int64_t cap_bytes) {
    DeviceScope dev__(sq ? sq->ctx : nullptr);
    if (!sq) return fail(CSDR_ESTATE, "squelch bank is null");
    if (!out) return fail(CSDR_EINVAL, "null argument");
    if (cap_bytes < (int64_t)sq->flags_h.size()) return fail(CSDR_ERANGE, "need room for %zu bytes", sq->flags_h.size());
    if (int rc = sq_flags(sq)) return rc;
    memcpy(out, sq->flags_h.data(), sq->flags_h.size());
    return CSDR_OK;
}

int squelch_bank_flags(csdr_squelch *sq, const csdr_bank *bank, const uint8_t **flags, int *max_slots, int *stride) {
    if (!sq) return fail(CSDR_ESTATE, "squelch bank is null");
    if (sq->src_bank != bank || sq->src_exec != bank->n_exec)
        return fail(CSDR_ESTATE, "the squelch bank's last process was not csdr_squelch_process_bank of this bank's last execute");
    if (int rc = sq_flags(sq)) return rc;
    *flags = sq->flags_h.data(); *max_slots = sq->max_slots; *stride = sq->max_blocks;
    return CSDR_OK;
}

extern "C" int csdr_squelch_device_items(csdr_squelch *sq, const csdr_squelch_item **dev, int *stride_items) {
    DeviceScope dev__(sq ? sq->ctx : nullptr);
    if (!sq) return fail(CSDR_ESTATE, "squelch bank is null");
    if (!dev) return fail(CSDR_EINVAL, "null argument");
    if (int rc = sq->hand_over()) return rc;               // whatever the caller enqueues on the boundary stream next reads the finished items
    *dev = sq->items.p;
    if (stride_items) *stride_items = sq->max_blocks;
    return CSDR_OK;
}

extern "C" int csdr_squelch_record(csdr_squelch *sq, int16_t *out_host, int64_t cap_samples, int64_t *offsets) {
    DeviceScope dev__(sq ? sq->ctx : nullptr);
    if (!sq) return fail(CSDR_ESTATE, "squelch bank is null");
    if (!offsets || cap_samples < 0 || (cap_samples > 0 && !out_host)) return fail(CSDR_EINVAL, "bad argument");
    const size_t S = (size_t)sq->max_slots;
    if (!sq->recorded) { std::fill(offsets, offsets + S + 1, (int64_t)0); return CSDR_OK; }
    CSDR_HIP_TRY(hipMemcpyAsync(offsets, sq->pack.p, (S + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, sq->st));
    CSDR_HIP_TRY(hipStreamSynchronize(sq->st));
    const int64_t total = offsets[S];
    if (total > cap_samples) return fail(CSDR_ERANGE, "need room for %lld samples", (long long)total);
    if (total > 0) {
        CSDR_HIP_TRY(hipMemcpyAsync(out_host, sq->pcm.p, (size_t)total * sizeof(int16_t), hipMemcpyDeviceToHost, sq->st));
        CSDR_HIP_TRY(hipStreamSynchronize(sq->st));
    }
    return CSDR_OK;
}
