// csdr_objects.hpp -- the object layouts behind the opaque handles of include/csdr_hip.h that more than one translation unit looks into
// (the demodulator bank reads the channelizer's output rotation; the audio / scope edges read the bank's slots).
#pragma once
#include <cmath>
#include <map>
#include <memory>
#include <vector>

#include "common.hpp"
#include "stream_order.hpp"
#include "design.hpp"
#include "kernels_post.hpp"
#include "kernels_chanfft.hpp"
#include "kernels_demod.hpp"
#include "kernels_digital.hpp"
#include "kernels_waterfall.hpp"

using namespace csdr;      // (this header is only included by the library's own translation units, all of which do the same)

// =================================================================================================== SDRPostThread
struct csdr_post {
    csdr_ctx *ctx = nullptr;
    bool configured = false;
    int mode = CSDR_POST_SINGLE, M = 1;
    int64_t sample_rate = 0, chan_bw = 0, chan_rate = 0, frequency = 0;
    int hop = 1;                             // input samples per output sample of a channel: M, M / 2 (PFBCH2) or 1 (single)
    int max_block_len = 0, max_blocks = 0;
    int64_t chan_stride = 0;                 // samples per channel row in `out` (even: rows stay 16-byte aligned)
    int n_blocks = 0, block_len = 0;         // of the last execute
    std::vector<int64_t> centers;            // chanCenters[M + 1]
    std::vector<int> active_host;            // sorted list of produced channels
    std::vector<int> row_order;              // csdr_post_set_row_order: channel of output row i (empty: row = channel).  A post with packed rows is a
                                             // time-slab PRODUCER: its buffer is the all-to-all's send buffer; no bank reads it, no DC blocker runs on it
    bool active_dirty = true;
    ChanGeom geom{};
    bool use_fft = false;                    // critically sampled, M = 2^a 3^b 5^c 7^d 11^e 13^f: chan_analyze_fft (kernels_chanfft.hpp)
    ChanFftGeom fgeom{};
    DevBuf<int> perm;                        // chan_analyze_fft: position after the last pass -> channel
    // `out` holds kPostBufs batches in rotation: the channelizer fills the next one while the demodulators still read
    // the previous (the reference hands ReBuffer blocks through a queue, SDRPostThread.cpp:341-396)
    static constexpr int kPostBufs = 3, kMaxConsumers = 4;
    int cur = 0;                             // buffer of the last execute
    uint64_t seq = 0;
    hipEvent_t ev_ready[kPostBufs] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_consumed[kPostBufs][kMaxConsumers] = {};
    int n_consumed[kPostBufs] = {0, 0, 0};
    DevBuf<float2> out, hist0, hist1, stage_in, twA, twB, twM, post2;
    DevBuf<float> taps;
    DevBuf<int> active;                      // [M] flags
    DevBuf<d2> dc_state, tile_end;           // dc_state[2]: ping-pong carried state
    int hist_parity = 0, dc_parity = 0;
    double dc_c = 0.0;                       // feedback coefficient of the DC blocker recurrence
    bool raw = false;                        // internal (zoomed spectrum view): SINGLE mode hands the input on unfiltered
    bool dc_enabled = true;                  // csdr_post_set_dc_blocker: a time-slab producer leaves channel 0 to the rank that owns it
    int import_k = -1;                       // buffer being assembled by csdr_post_import_begin .. commit
    bool rotate = false;                     // the output is read from a stream that is no lane (csdr_post_exchange_rows_begin's transfers): the buffers rotate whatever the stream folding
    std::map<std::vector<int>, int *> rowlists;   // device copies of the channel lists export / import calls name (a handful, reused every batch)
};
static inline float2 *post_buf(const csdr_post *p, int k) { return p->out.p + (size_t)k * p->chan_stride * p->M; }

// =================================================================================================== demodulator bank
namespace csdr {
struct DigSlot;                              // a digital slot's modem (csdr_digital.hip)
struct SlotHost {
    bool configured = false, active = false;
    csdr_demod_params prm{};
    design::MsresampPlan iq, au;
    int64_t chan_rate = 0;
    // integer state mirrored on the host (closed-form bookkeeping)
    uint32_t theta = 0, dtheta = 0, buf_idx = 0, phase = 0, aphase = 0, abuf = 0, ssb_theta = 0, cw_dtheta = 0;
    uint32_t tab_rot = 0;                    // layout of the oscillator table in the front-end's LDS for this dtheta (fe_table_rotation)
    long long shift_frequency = 0;
    bool shift_valid = false;
    int hist_parity = 0, last_parity = 0;
    int prev_J = 0;                          // resampled-IQ samples of the previous executed batch
    // routing of the last batch: getChannelAt is a scan over M + 1 centres (1 M comparisons per batch with 1024 demodulators behind M = 1024);
    // the centres are a function of (post frequency, sample rate, M): same key, same channel
    int64_t route_freq = 0, route_post_freq = 0, route_post_rate = 0;
    int route_M = 0, route_ch = -2;          // -2: nothing cached
    int warm = 0;                            // cascade span in input samples (+ one output period)
    bool fms_sos_set = false;                // csdr_bank_set_fms_pilot: caller-supplied pilot band-pass sections
    float fms_b[15] = {0}, fms_a[15] = {0};
    void *slab = nullptr;
    SlotCfg cfg{};
    // results of the last execute
    std::vector<csdr_block_result> results;
    int last_J = 0, last_A = 0;
    int last_ash = -1;                       // floats per audio-arbitrary output of the last execute = 2^last_ash; -1: no audio stage ran
    std::shared_ptr<DigSlot> dig;           // CSDR_MODEM_DIGITAL: the decision stage behind the front-end
};
// a designed msresamp as the kernels read it (the demodulator bank's slots; the view bank's resamplers)
static inline void fill_resamp_cfg(ResampCfg &rc, const design::MsresampPlan &p, int arms_idx) {
    memset(&rc, 0, sizeof rc);
    rc.interp = p.interp ? 1 : 0;
    rc.S = (int)p.S;
    rc.step = p.step;
    rc.arms_idx = arms_idx;
    for (unsigned e = 0; e < p.S; ++e) {
        // execution order: decimator runs design index S-1 first; interpolator runs design index 0 first
        const unsigned g = p.interp ? e : (p.S - 1 - e);
        rc.m_x[e] = (int)p.m[g];
        for (unsigned j = 0; j < p.m[g]; ++j) rc.h_x[e][j] = p.h1[g][j];
    }
}
// the base twiddle table exp(-2 pi i k / n) that lds_fft and the spectrum chain read (n = kTwTab of kernels_spec.hpp), on the device once per object
static inline int upload_twiddles(DevBuf<float2> &tw, int n) {
    if (tw.p) return CSDR_OK;
    std::vector<float2> t((size_t)n);
    for (int i = 0; i < n; i++) { const double a = -2.0 * M_PI * i / n; t[(size_t)i] = make_float2((float)std::cos(a), (float)std::sin(a)); }
    if (int rc = tw.reserve((size_t)n)) return rc;
    CSDR_HIP_TRY(hipMemcpy(tw.p, t.data(), (size_t)n * sizeof(float2), hipMemcpyHostToDevice));
    return CSDR_OK;
}
constexpr int kStageRing = 4;                // pinned staging sets for the per-batch uploads
}  // namespace csdr

struct csdr_bank {
    csdr_ctx *ctx = nullptr;
    int max_demods = 0, max_blocks = 0;
    std::vector<SlotHost> slots;
    DevBuf<SlotCfg> cfgs;
    // per-batch device tables, two copies: the front-end of batch i+1 uploads its set while the audio kernels of batch i
    // still read theirs
    // ONE table per copy, uploaded by one transfer per batch (three transfers were three stream round trips: 75 us of a 0.65 ms C4 batch):
    //   SlotDyn [max_demods] | int [3][max_demods]: all running slots | running auto-gain slots | grouped by front-end kernel | BlockPlan [max_demods][blocks + 1]
    DevBuf<char> tables;                     // [2][table_bytes]
    size_t table_bytes = 0, off_lists = 0, off_plans = 0;
    SlotDyn *dyns_of(char *t) const { return reinterpret_cast<SlotDyn *>(t); }
    int *lists_of(char *t) const { return reinterpret_cast<int *>(t + off_lists); }
    BlockPlan *plans_of(char *t) const { return reinterpret_cast<BlockPlan *>(t + off_plans); }
    uint64_t seq = 0;
    hipEvent_t ev_fe_done[2] = {nullptr, nullptr}, ev_audio_done[2] = {nullptr, nullptr};
    bool audio_pending[2] = {false, false};
    ReadGate tables_read[2];                 // behind the audio kernels of a batch: the device tables of its parity may be refetched (by the channelizer's stream)
    DevBuf<float> arms;
    DevBuf<ModemConsts> mconsts;
    PinBuf<char> tables_h[kStageRing];
    hipEvent_t stage_ev[kStageRing] = {nullptr, nullptr, nullptr, nullptr};
    bool stage_used[kStageRing] = {false, false, false, false};
    int stage_next = 0;
    PinBuf<BlockOut> bout_h;
    std::map<uint32_t, int> arm_index;       // key: bit pattern of rate_arb
    std::vector<float> arms_host;
    int n_run = 0, last_nb = 0;
    size_t lds_attr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // the front-end launch lists of the last batch and what they were built from (slot, channel, cascade class per running slot): csdr_bank_execute
    std::vector<int> grp_key, grp_key_scratch, grp_list;
    int grp_off[8] = {0}, grp_n[8] = {0}, grp_rows[8] = {0};
    bool grp_merged56 = false;
    struct SnapBytes { char b[64]; };
    std::vector<SnapBytes> snap;             // host-state snapshot of a batch being planned (a rejected batch puts it back)
    DevBuf<int16_t> pcm;                     // csdr_bank_fetch_pcm16: the converted audio of one slot
    DevBuf<PcmJob> pcm_jobs;
    std::vector<int> dig_run;                // digital slots of the batch being planned (csdr_digital.hip)
    DevBuf<char> dig_jobs;                   // their launch records
    std::vector<char> dig_jobs_h;
    DevBuf<GmskJob> gmsk_jobs;               // the GMSK slots' launch records
    std::vector<GmskJob> gmsk_jobs_h;
    DevBuf<TableJob> tab_jobs;               // the table slots' launch records
    std::vector<TableJob> tab_jobs_h;
    // readers that stay on the device, each behind a gate of its own (stream_order.hpp); a bank nobody reads this way never has their events.
    // The slots' resampled IQ (bank_iq_acquire / _release: the spectrum bank on its own stream), by parity of the batch that was read
    ReadGate iq[2];
    // the slots' audio and scope taps (bank_audio_acquire / _release: the scope bank on its own stream).  SlotCfg::audio and ::scope are
    // single-buffered: the NEXT execute's modem / audio lane waits for the readers
    ReadGate audio;
    // a batch's block plan in the device tables (bank_plan_release: the squelch bank), by parity of the batch that was read: the execute that
    // refetches that copy of the tables -- the second one after -- waits for the readers
    ReadGate plan[2];
    uint64_t n_exec = 0;                         // csdr_bank_execute calls that got as far as clearing the slots' results: what a reader of "the last execute" was taken from
};

// =================================================================================================== spectrum points for device-side readers
// The display points of a spectrum's last process, for a reader that stays in HBM (csdr_waterfall_step_spec): `reader` is made to wait for the
// averaging lane's enqueued work by an event (no host synchronisation); after enqueueing its reads the reader calls spec_points_release, and the
// spectrum's next process waits for them before it rewrites the buffer.  (csdr_spec.hip)
struct SpecPointsRef {
    csdr_ctx *ctx = nullptr;
    const float *points = nullptr;           // [frames][F]: the y of every point
    int F = 0, frames = 0;
    HideDcSpan dc;                           // csdr_spec_set_hide_dc: what csdr_spec_fetch would overwrite (empty when off)
};
int spec_points_acquire(csdr_spec *s, hipStream_t reader, SpecPointsRef *out);
int spec_points_release(csdr_spec *s, hipStream_t reader);
csdr_ctx *spec_ctx(const csdr_spec *s);      // the context a spectrum was created on (csdr_spec_process_distrib checks it against the distributor's)

// The spectrum bank's counterpart (csdr_wfbank_step_specbank): the points of every slot's frames of the bank's last process, [slot][max_frames][F],
// with the same two events.  The spectrum bank's next process, process_bank, setup or reset_slot waits for the reader before it touches them.
// (csdr_specbank.hip; the frames of a slot are csdr_specbank_frames)
struct SpecBankPointsRef {
    csdr_ctx *ctx = nullptr;
    const float *points = nullptr;           // frame f of slot s: points + ((size_t)s * max_frames + f) * F
    int F = 0, max_slots = 0, max_frames = 0;
};
int specbank_points_acquire(csdr_specbank *sb, hipStream_t reader, SpecBankPointsRef *out);
int specbank_points_release(csdr_specbank *sb, hipStream_t reader);

// =================================================================================================== resampled IQ for device-side readers
// The bank-side counterpart of the above: the slots' resampled IQ of the last execute (where csdr_bank_fetch_iq reads it), for a reader that stays in
// HBM (csdr_specbank_process_bank).  `reader` is made to wait for the front-end of that execute by an event (no host synchronisation); after enqueueing
// its reads the reader calls bank_iq_release, and the execute that rewrites that parity's buffers -- the second one after -- waits for them.  (csdr_bank.hip)
int bank_iq_acquire(csdr_bank *b, hipStream_t reader);
int bank_iq_release(csdr_bank *b, hipStream_t reader);
// block bb of a slot's last execute inside that buffer: the samples in front of it are the earlier blocks' (BlockPlan::j0, batch-relative from 0)
static inline const float2 *bank_slot_iq(const SlotHost &s) { return s.cfg.iq + (size_t)s.last_parity * ((size_t)kIqHist + s.cfg.cap_iq) + kIqHist; }

// =================================================================================================== audio and scope taps for device-side readers
// The audio side's counterpart: the slots' audio and scope taps of the last execute (where csdr_bank_scope_frame points), for a reader that stays in
// HBM (csdr_scopebank_process_bank).  `reader` is made to wait for the modem / audio kernels of that execute by an event (no host synchronisation);
// after enqueueing its reads the reader calls bank_audio_release, and the very next execute -- these buffers are single -- makes its modem / audio
// lane wait for them before it rewrites the taps.  (csdr_bank.hip)
int bank_audio_acquire(csdr_bank *b, hipStream_t reader);
int bank_audio_release(csdr_bank *b, hipStream_t reader);
// The block plan of the last execute that ran a slot, where it lies in the device tables: slot s at bank_last_plans(b) + s * (last_nb + 1).  It was
// fetched on the front-end's lane in front of the kernels bank_audio_acquire orders the reader behind; after enqueueing its reads the reader calls
// bank_plan_release, and the execute that refetches that copy of the tables waits for them.  (csdr_bank.hip)
static inline const BlockPlan *bank_last_plans(const csdr_bank *b) { return b->plans_of(b->tables.p + (size_t)((b->seq - 1) & 1) * b->table_bytes); }
int bank_plan_release(csdr_bank *b, hipStream_t reader);

// =================================================================================================== squelch flags for the mixer
// The flags of the squelch bank's last process, [max_slots][stride] on the host (csdr_squelch_fetch_flags' copy, cached until the next process), for
// csdr_mix_push_squelched: CSDR_ESTATE unless that process was csdr_squelch_process_bank of `bank`'s last execute.  (csdr_squelch.hip)
int squelch_bank_flags(csdr_squelch *sq, const csdr_bank *bank, const uint8_t **flags, int *max_slots, int *stride);

// internal modem id: NCO + msresamp only, no modem / audio stage (the zoomed spectrum view's shift + resample, SpectrumVisualProcessor.cpp:306-379)
#define CSDR_MODEM_FRONTEND_ONLY 100
// csdr_bank_configure_slot without the public entry point's modem-range check (csdr_bank.hip; the zoomed view configures a front-end-only slot)
int bank_configure_slot(csdr_bank *b, int slot, const csdr_demod_params *prm, const csdr_post *post);
static inline bool is_fe_only(int modem) { return modem == CSDR_MODEM_FRONTEND_ONLY || modem == CSDR_MODEM_HOST || modem == CSDR_MODEM_DIGITAL; }
// digital slots (csdr_digital.hip): csdr_bank_execute plans each one's batch while it walks the slots (plan = the slot's block starts, NB + 1 of
// them; nullptr: the slot is skipped this batch), and launches the decision kernel behind the front-end, on the modem / audio lane
void bank_digital_plan(csdr_bank *b, int slot, int NB, const BlockPlan *plan);
int bank_digital_launch(csdr_bank *b, const BlockPlan *plans_d, int NB);
