/*
 * csdr_hip.h -- C ABI of the MI355X-native streaming-IQ DSP hot path of CubicSDR.
 *
 * The reference (cjcliffe/CubicSDR v0.2.8) has no FFI: its hot path is C++ classes calling liquid-dsp
 * (SURVEY.md section 8b).  This header is the boundary a maintainer binds from those classes; every entry
 * point names the reference code it replaces (file:line relative to the reference tree).  Plain pointers
 * and sizes only; every call returns 0 on success or a negative CSDR_E* code and never throws.  A handle
 * must be used from one thread at a time (same rule as the reference objects: one owning IOThread each); different
 * handles of one context may be used from different threads at once -- the reference's thread cut: SDRPostThread with
 * its demodulators (csdr_post + csdr_bank: a call that takes two handles uses both) beside the spectrum thread (csdr_spec).
 *
 * Sample format everywhere: interleaved complex float32 {re, im} (liquid_float_complex, liquid.h:149-157).
 * (A radio's native integer formats enter through the raw ingest, which widens them to that on the GPU: see "ingest of a radio's native sample format".)
 * "dev" pointers are HIP device pointers resident in HBM; "host" pointers are ordinary host memory.
 *
 * Batching: the reference handles one SDRThreadIQData block per loop turn (60 blocks/s,
 * SoapySDRThread.cpp:12,668-674).  Every *_execute call here takes `n_blocks` consecutive blocks of
 * `block_len` samples and produces exactly the per-block results the reference would produce for that
 * sequence (per-block output counts included); n_blocks = 1 is the real-time case.
 */
#ifndef CSDR_HIP_H
#define CSDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSDR_OK            0
#define CSDR_EINVAL       -1   /* bad argument / unsupported parameter */
#define CSDR_ENOMEM       -2   /* host or device allocation failed */
#define CSDR_EHIP         -3   /* a HIP runtime call failed (see csdr_last_error) */
#define CSDR_ESTATE       -4   /* object not configured / wrong call order */
#define CSDR_ERANGE       -5   /* capacity exceeded (block too long, too many demods, ...) */
#define CSDR_EUNSUPPORTED -6   /* valid in the reference, not built yet (see DESIGN.md out-of-scope) */

typedef struct csdr_ctx   csdr_ctx;    /* device + stream */
typedef struct csdr_post  csdr_post;   /* SDRPostThread's arithmetic: DC blocker | firpfbch channelizer */
typedef struct csdr_bank  csdr_bank;   /* N x {DemodulatorPreThread + DemodulatorThread + Modem} arithmetic */
typedef struct csdr_spec  csdr_spec;   /* SpectrumVisualProcessor's arithmetic */
typedef struct csdr_scope csdr_scope;  /* ScopeVisualProcessor's arithmetic (audio scope + audio spectrum) */
typedef struct csdr_mix   csdr_mix;    /* AudioThread's mixing callback, PCM conversion */
typedef struct csdr_ingest csdr_ingest; /* page-locked block ring -> HBM, one transfer per block */
typedef struct csdr_comm  csdr_comm;   /* one IQ stream over the GPUs of a node: RCCL over xGMI */
typedef struct csdr_waterfall csdr_waterfall; /* WaterfallPanel's arithmetic: quantised lines, two ring textures, themed RGBA */
typedef struct csdr_distrib csdr_distrib; /* FFTDataDistributor's line cutting: the waterfall feed, cut where the block lies in HBM */
typedef struct csdr_specbank csdr_specbank; /* N x SpectrumVisualProcessor, one per demodulator: every slot and block of an execute in one launch */
typedef struct csdr_wfbank csdr_wfbank;     /* N x WaterfallPanel, one per demodulator: every slot of a step, an update or a render in one launch */
typedef struct csdr_scopebank csdr_scopebank; /* N x ScopeVisualProcessor, one per demodulator: every slot and frame of a call in two launches */
typedef struct csdr_squelch csdr_squelch;     /* N x DemodulatorThread's level, floor, ceiling and squelch: every slot and block of an execute in one launch */
typedef struct csdr_viewbank csdr_viewbank;   /* N x SpectrumVisualProcessor in zoomed view, one per demodulator: every slot and input of a call in one launch */
typedef struct csdr_tracebank csdr_tracebank; /* the spectrum, hold and scope lines of any number of items as tiles of one RGBA8 atlas */
typedef struct csdr_overlay csdr_overlay;     /* ordered primitive lists -- grid, ticks, markers, glyphs -- composited onto the tiles of an atlas in one launch */
typedef struct csdr_density csdr_density;     /* N hit grids in HBM: how often the trace passed through every pixel of a tile, drawn through a palette */

/* ------------------------------------------------------------------ context */
int         csdr_abi_version(void);
const char *csdr_strerror(int code);
const char *csdr_last_error(void);                 /* thread-local detail string of the last failure */

/* Streams.  The reference runs one IOThread per stage (SDRPostThread, DemodulatorPreThread/DemodulatorThread per
 * demodulator, SpectrumVisualDataThread) joined by queues, so block i+1 is channelized while block i is demodulated.
 * The ctx mirrors that with one internal HIP stream per stage (channelizer, demodulator front-end, modem + audio,
 * spectrum FFT, spectrum averaging + display); events order the hand-offs and the buffer rotations, so consecutive
 * *_execute / *_process calls overlap on the device and every call returns as soon as its work is enqueued.
 * `hip_stream` is the BOUNDARY stream: an existing hipStream_t (e.g. PyTorch's current stream) on which the caller
 * produces device-resident IQ -- every execute first waits for what is enqueued there -- or NULL for a private one.
 * csdr_ctx_join makes the boundary stream wait for everything enqueued so far (for consumers chained on it);
 * csdr_ctx_synchronize blocks the host until all of it is done.  The fetch / read calls synchronise what they need.
 * The device's NULL (default) stream has the handle 0 and cannot be told from "no stream" by its value: pass CSDR_STREAM_NULL to
 * make it the boundary stream (e.g. PyTorch's default stream, whose raw handle is 0). */
#define CSDR_STREAM_NULL ((void *)(intptr_t)-1)
int  csdr_ctx_create(int device, void *hip_stream, csdr_ctx **out);
int  csdr_ctx_owns_stream(const csdr_ctx *ctx);    /* 1: the boundary stream is private (created by csdr_ctx_create), 0: the caller's */
void csdr_ctx_destroy(csdr_ctx *ctx);
int  csdr_ctx_synchronize(csdr_ctx *ctx);
int  csdr_ctx_join(csdr_ctx *ctx);
void *csdr_ctx_stream(csdr_ctx *ctx);              /* the boundary hipStream_t */
/* HIP-event timer (bench.py roofline leg): start / stop marks on the boundary stream, joined with every internal
 * stream on both sides, so the bracket covers exactly the work enqueued between the two calls; returns milliseconds. */
int  csdr_ctx_timer_start(csdr_ctx *ctx);
int  csdr_ctx_timer_stop(csdr_ctx *ctx, float *ms);
/* Optional per-kernel profile: while enabled (on = 1) every kernel launch of this ctx -- or, with on = P > 1, every P-th
 * launch of each kernel -- is bracketed by HIP events on the stream it is launched on; fetch returns the accumulated
 * device time and the number of bracketed launches of kernel `id`. */
int  csdr_ctx_profile_enable(csdr_ctx *ctx, int on);
int  csdr_ctx_profile_num_kernels(void);
const char *csdr_ctx_profile_kernel_name(int id);
int  csdr_ctx_profile_fetch(csdr_ctx *ctx, int id, double *total_ms, int64_t *launches);
/* ALL launches of kernel `id` since the profile was enabled, bracketed or not (launches per batch = this / batches) */
int  csdr_ctx_profile_launches(csdr_ctx *ctx, int id, int64_t *launches);
/* shortest / longest bracketed launch of kernel `id` since the profile was enabled (the spread behind csdr_ctx_profile_fetch's mean: a kernel
   whose duration moves with the clocks or the placement of its buffers shows it here); both 0 when nothing was bracketed */
int  csdr_ctx_profile_range(csdr_ctx *ctx, int id, double *min_ms, double *max_ms);
/* raw device memory for callers without a GPU array library (tests written in C/C++) */
int  csdr_dev_alloc(csdr_ctx *ctx, uint64_t bytes, void **dev);
int  csdr_dev_free(csdr_ctx *ctx, void *dev);
int  csdr_dev_upload(csdr_ctx *ctx, void *dev, const void *host, uint64_t bytes);
int  csdr_dev_download(csdr_ctx *ctx, void *host, const void *dev, uint64_t bytes);
/* Page-lock a caller-owned host buffer (e.g. the pooled SDRThreadIQData blocks, SoapySDRThread.cpp:221-225) so that the
 * host-to-device copies of csdr_post_execute / csdr_spec_process read it by DMA; unregister before freeing it. */
int  csdr_host_register(csdr_ctx *ctx, void *host, uint64_t bytes);
int  csdr_host_unregister(csdr_ctx *ctx, void *host);

/* ------------------------------------------------------------------ SDRPostThread (src/sdr/SDRPostThread.cpp)
 * replaces: iirfilt_crcf_create_dc_blocker :29, runSingleCH :248-299 (iirfilt_crcf_execute_block :284),
 * initPFBCH :401-414 (firpfbch_crcf_create_kaiser(ANALYZER,M,4,60) :406, chanBw = sampleRate/numChannels :408),
 * runPFBCH :416-455 (firpfbch_crcf_analyzer_execute :449-451), de-interleave + channel-0 DC block :364-382,
 * updateChannels :116-124, getChannelAt :128-139. */
#define CSDR_POST_SINGLE 0   /* numChannels == 1 : DC-blocked full-rate stream is "channel 0" */
#define CSDR_POST_PFBCH  1   /* SDRPostPFBCH  (SDRPostThread.h:9-12), critically sampled analyzer */
#define CSDR_POST_PFBCH2 2   /* SDRPostPFBCH2: initPFBCH2 :458-470 (firpfbch2_crcf_create_kaiser(ANALYZER,M,4,60) :463),
                              * runPFBCH2 :472-512 (firpfbch2_crcf_execute per M/2 inputs :505-507): every channel comes
                              * out at 2*chanBw (runDemodChannels(chanBw * 2) :510), channel centres are unchanged */

int  csdr_post_create(csdr_ctx *ctx, csdr_post **out);
void csdr_post_destroy(csdr_post *post);
/* (re)build for a sample rate / channel count; resets filter state like initPFBCH(). max_* size the HBM buffers. */
int  csdr_post_configure(csdr_post *post, int64_t sample_rate, int num_channels, int mode,
                         int max_block_len, int max_blocks);
/* Process n_blocks x block_len input samples (block_len % num_channels == 0).  `iq` is device memory when
 * iq_is_dev != 0, else host memory that is copied to a device staging buffer with hipMemcpyAsync on the stage's stream: from
 * pageable memory the runtime stages the copy before the call returns; from page-locked memory (csdr_host_register) it is a
 * DMA that may still be in flight, so the buffer must stay unchanged until the next synchronising call on this object
 * (csdr_post_read_channel, csdr_bank_fetch_*, csdr_ctx_synchronize).  Output stays in HBM, channel-major. */
int  csdr_post_execute(csdr_post *post, const float *iq, int iq_is_dev, int n_blocks, int block_len,
                       int64_t frequency);
/* Optional: produce only these channels (the reference skips channels without consumers, :336-339).  NULL = all.
 * The wrap channel index M is accepted as an alias of M/2. */
int  csdr_post_set_active_channels(csdr_post *post, const int *channels, int n);
int64_t csdr_post_channel_bandwidth(const csdr_post *post);                  /* chanBw (:408) */
int64_t csdr_post_channel_rate(const csdr_post *post);                       /* sampleRate stamped on the channel data (:344): chanBw, 2*chanBw for PFBCH2 */
int     csdr_post_num_channels(const csdr_post *post);
const char *csdr_post_kernel_name(const csdr_post *post);                    /* diagnostic: the kernel runPFBCH's transform (:449-451) maps to for this channel count: "dc_blocker" (single channel), "chan_analyze_p2" (M = 2 * prime <= 122; firpfbch2 with M / 2 odd, 38 <= M <= 126), "chan_analyze_fft" (small factors, one prime factor 29 .. 509; firpfbch2 with M % 4 == 0), "chan_analyze" (any other even M) */
int64_t csdr_post_channel_center(const csdr_post *post, int i);              /* chanCenters[i], i in [0, M] (:116-124) */
int     csdr_post_channel_at(const csdr_post *post, int64_t frequency);      /* getChannelAt (:128-139) */
/* copy one channel's samples of the last execute to the host (tests / demod-visual tap); ch == M is the wrap
 * channel (alias of M/2, :359-361).  *n receives the number of complex samples written. */
int  csdr_post_read_channel(csdr_post *post, int ch, float *host_out, int cap_samples, int *n);
/* Time-slab sharding of ONE stream over several GPUs (SURVEY 8e option 2: each rank channelizes ITS blocks of a batch for all
 * channels; an all-to-all gives every rank the full time series of the channels its demodulators sit on).  No reference
 * counterpart: SDRPostThread runs on one thread.  Producer side: csdr_post_set_history (the csdr_post_history_length() input samples
 * in front of the slab, device pointer; fewer = zeros in front), csdr_post_set_dc_blocker(0) (channel 0's DC blocker, SDRPostThread.cpp:375,
 * is a recurrence over the whole stream: the owner of channel 0 runs it), csdr_post_execute, csdr_post_export_rows (rows of the listed
 * channels of the last execute -> dst_dev[i * dst_stride + frame], complex float).  Owner side, on a second post object configured alike:
 * csdr_post_import_begin, csdr_post_import_rows per peer (its frames at frame0), csdr_post_import_commit; then csdr_bank_execute. */
int  csdr_post_history_length(const csdr_post *post);
/* producer only: store the rows of the listed channels one after the other in THIS order (row i = channels[i]; other channels are not
 * produced; n = 0: back to "row = channel").  With the channels grouped by owning rank the output buffer IS the all-to-all's send buffer:
 * csdr_post_exchange_rows then sends it as it stands (no export copy).  Such a post cannot feed a bank or run the DC blocker. */
int  csdr_post_set_row_order(csdr_post *post, const int *channels, int n);
int  csdr_post_set_history(csdr_post *post, const float *dev_tail, int64_t n_samples);
int  csdr_post_set_dc_blocker(csdr_post *post, int enabled);
int  csdr_post_export_rows(csdr_post *post, const int *channels, int n, float *dst_dev, int64_t dst_stride);
int  csdr_post_import_begin(csdr_post *post, int n_blocks, int block_len, int64_t frequency);
int  csdr_post_import_rows(csdr_post *post, const int *channels, int n, const float *src_dev, int64_t src_stride, int64_t frame0, int64_t n_frames);
int  csdr_post_import_commit(csdr_post *post);

/* ------------------------------------------------------------------ demodulator bank
 * One slot == one DemodulatorInstance's DSP state: NCO shift + msresamp_crcf decimator
 * (src/demod/DemodulatorPreThread.cpp:154-209, built by DemodulatorWorkerThread.cpp:63-101), the modem
 * (src/modules/modem/analog/Modem{NBFM,FM,AM,USB,LSB}.cpp ::demodulate), ModemAnalog::buildAudioOutput
 * (ModemAnalog.cpp:67-93) and the level / peak measurements of DemodulatorThread::run
 * (DemodulatorThread.cpp:142-152,223-233). */
#define CSDR_MODEM_NBFM 0   /* ModemNBFM.cpp:26-39  freqdem kf=0.5, no auto-gain */
#define CSDR_MODEM_FM   1   /* ModemFM.cpp:26-39    same arithmetic, 200 kHz default bandwidth */
#define CSDR_MODEM_AM   2   /* ModemAM.cpp:29-50    |x| -> 51-tap DC notch, auto-gain */
#define CSDR_MODEM_USB  3   /* ModemUSB.cpp:43-64   fs/4 shift, 6th-order Butterworth, Hilbert, upper sideband */
#define CSDR_MODEM_LSB  4   /* ModemLSB.cpp         mirror of USB, lower sideband */
#define CSDR_MODEM_CW   6   /* ModemCW.cpp:155-209  msresamp_cccf interpolation to the audio rate, 650 Hz beep oscillator, c2r Hilbert
                             * (upper sideband), auto-gain in dB; bandwidth floor 500 Hz (:100-104) */
#define CSDR_MODEM_DSB  7   /* ModemDSB.cpp:38-53   ampmodem(0.5, DSB, suppressed carrier): Costas loop around the table oscillator
                             * (a per-sample feedback loop: one thread per demodulator walks the batch), auto-gain */
#define CSDR_MODEM_IQ   5   /* ModemIQ.cpp:41-61    stereo pass-through of the resampled IQ (L = imag, R = real); the
                             * bandwidth is forced to the audio rate (checkSampleRate :31-33); 2 floats per IQ sample */

#define CSDR_MODEM_FMS  8   /* ModemFMStereo.cpp:178-287  FM stereo: pilot band-pass + PLL, L-R down-mix, two audio resamplers, de-emphasis */
#define CSDR_MODEM_HOST 9   /* a modem registered through Modem::addModemFactory whose demodulate() is host code (Modem.h:127-166): the slot runs
                             * DemodulatorPreThread's arithmetic only (NCO shift + msresamp_crcf to `bandwidth`); the block's resampled IQ is
                             * fetched with csdr_bank_fetch_iq and handed to the plug-in's demodulate(kit, iq, audioOut) on the host.
                             * n_audio / level / peak of the block results stay 0: they are the plug-in's to produce. */

typedef struct csdr_demod_params {
    int32_t modem;             /* CSDR_MODEM_* (DemodulatorInstance::setDemodulatorType) */
    int32_t bandwidth;         /* Hz, modem input rate after checkSampleRate() (setBandwidth) */
    int32_t audio_sample_rate; /* Hz (setAudioSampleRate; 48000 in the reference, DemodulatorInstance.cpp:345) */
    int32_t modem_arg;         /* FM stereo: de-emphasis in microseconds ("demph", ModemFMStereo.cpp:42-81; 0 = the default 75, < 0 = none); else 0 */
    int64_t frequency;         /* Hz, demodulator centre (setFrequency) */
} csdr_demod_params;

/* per (slot, block) results, fetched after csdr_bank_execute */
typedef struct csdr_block_result {
    int32_t  n_iq;          /* samples written by msresamp_crcf_execute for this block (numWritten, :209) */
    int32_t  n_audio;       /* numAudioWritten (ModemAnalog.cpp:88) */
    int32_t  audio_offset;  /* offset of this block's audio inside the slot's audio buffer of this execute */
    int32_t  skipped;       /* 1 when the block was skipped by the |shift| > 0.75*rate rule (:161-165) */
    double   level_accum;   /* sum of |x| (IQ for NBFM/FM, audio for AM/USB/LSB: useSignalOutput) */
    int32_t  level_count;   /* number of terms in level_accum */
    float    audio_peak;    /* max |audio| (DemodulatorThread.cpp:223-233) */
    uint32_t nco_theta;     /* NCO phase word after the block (bit-exact item) */
    uint32_t resamp_phase;  /* arbitrary-resampler 24-bit phase after the block (bit-exact item) */
    uint32_t buffer_index;  /* msresamp half-band input buffer fill after the block (bit-exact item) */
    uint32_t reserved;
} csdr_block_result;

int  csdr_bank_create(csdr_ctx *ctx, int max_demods, int max_blocks, csdr_bank **out);
void csdr_bank_destroy(csdr_bank *bank);
/* (Re)build slot `slot` (MAKE_DEMOD / BUILD_FILTERS of DemodulatorWorkerThread.cpp:40-101): designs the filters
 * on the host for the CURRENT channel rate of `post` and resets the slot's state, like the worker thread
 * handing over a fresh msresamp/modem/kit.  Changing only `frequency` later: csdr_bank_set_frequency. */
int  csdr_bank_configure_slot(csdr_bank *bank, int slot, const csdr_demod_params *p, const csdr_post *post);
int  csdr_bank_set_frequency(csdr_bank *bank, int slot, int64_t frequency);
int  csdr_bank_set_active(csdr_bank *bank, int slot, int active);
/* Route every active slot to its channel of `post`'s last execute (runDemodChannels :303-398) and run
 * NCO + decimator + modem + audio resampler for all of them, all blocks, in a handful of launches. */
int  csdr_bank_execute(csdr_bank *bank, const csdr_post *post);
/* results of the last execute (blocks in order); synchronises the stream */
int  csdr_bank_fetch_results(csdr_bank *bank, int slot, csdr_block_result *out, int cap_blocks, int *n_blocks);
int  csdr_bank_fetch_audio(csdr_bank *bank, int slot, float *host_out, int cap_samples, int *n);
int  csdr_bank_fetch_iq(csdr_bank *bank, int slot, float *host_out, int cap_samples, int *n);   /* resampled IQ */
/* ModemAnalog::getDemodOutputData() of the LAST block of the last execute (ModemAnalog.cpp:95-97): the gain-scaled demodulator
 * output in front of the audio resampler, at most DEMOD_VIS_SIZE = 2048 samples (DemodulatorThread.h:15) -- what the scope tap
 * hands to the audio scope when the audio is decimated (DemodulatorThread.cpp:293-305).  *n = 0 for the I/Q and CW modems. */
int  csdr_bank_fetch_demod_output(csdr_bank *bank, int slot, float *host_out, int cap_samples, int *n);
/* FM stereo (CSDR_MODEM_FMS).  The 19 kHz pilot band-pass is iirfilt_crcf_create_prototype(CHEBY2, BANDPASS, SOS, 5, 19500/fs, 19000/fs, 1, 60)
 * (ModemFMStereo.cpp:128-139): csdr_design_fms_pilot returns the five sections the library designs for a modem input rate
 * (b15 / a15: three taps per section, execution order); csdr_bank_set_fms_pilot replaces a slot's sections (NULL: back to the design) --
 * e.g. with the host liquid's own liquid_iirdes output, whose last-place roundings depend on its libm;
 * csdr_bank_fetch_fms_stage returns intermediates of the last batch for stage-by-stage checks (which = 0: pilot oscillator phase
 * words, uint32 per resampled-IQ sample; 1: the stereo-difference stream before its audio resampler, float). */
int  csdr_design_fms_pilot(int64_t sample_rate, float *b15, float *a15);
int  csdr_bank_set_fms_pilot(csdr_bank *bank, int slot, const float *b15, const float *a15);
int  csdr_bank_fetch_fms_stage(csdr_bank *bank, int slot, int which, void *host_out, int cap_samples, int *n);
/* device-side total of audio samples produced by the last execute over all slots (bench sanity) */
int  csdr_bank_total_audio(csdr_bank *bank, int64_t *n);

/* ------------------------------------------------------------------ digital lab (src/modules/modem/digital/, ENABLE_DIGITAL_LAB)
 * A digital slot runs DemodulatorPreThread's arithmetic (NCO shift + msresamp_crcf to the modem rate, as any slot) and then the modem's
 * hard decisions: one per resampled IQ sample for the modemcf constellations (ModemPSK.cpp:108-118 and alike: no symbol timing), one per
 * k = rate / sps samples for FSK (ModemFSK.cpp:127-143, the samples short of a symbol carried to the next block).  No audio: n_audio, level
 * and peak of its csdr_block_result stay 0.  GMSK (ModemGMSK.cpp:116-134) runs gmskdem per sps samples of each block as the reference frames them:
 * I = ceil((c + n) / sps / sps) symbols from the block's start, c = kit->inputBuffer.size() (samples past the block's end read as zero).
 * APSK, SQAM and V.29 (ModemST) -- and liquid's whole `arb` family -- run as TABLE slots (below): their points are liquid's own tables, which the
 * product does not carry; the caller, who has liquid linked, reads them through modemcf_modulate and hands them over as data. */
#define CSDR_MODEM_DIGITAL 10        /* configured only through csdr_bank_configure_digital_slot */
#define CSDR_DIGITAL_PSK   0         /* ModemPSK   modemcf PSK2..PSK256, lock at EVM <= 0.005 */
#define CSDR_DIGITAL_DPSK  1         /* ModemDPSK  modemcf DPSK2..DPSK256, 0.005 */
#define CSDR_DIGITAL_ASK   2         /* ModemASK   modemcf ASK2..ASK256, 0.005 */
#define CSDR_DIGITAL_QAM   3         /* ModemQAM   modemcf QAM4..QAM256 (square and rectangular), 0.5 */
#define CSDR_DIGITAL_BPSK  4         /* ModemBPSK, 0.005 */
#define CSDR_DIGITAL_QPSK  5         /* ModemQPSK, 0.8 */
#define CSDR_DIGITAL_OOK   6         /* ModemOOK, 0.005 */
#define CSDR_DIGITAL_FSK   7         /* ModemFSK   fskdem(bps, rate / sps, bw); no lock (the reference never updates it) */
#define CSDR_DIGITAL_GMSK  8         /* ModemGMSK  gmskdem(sps, fdelay, ebf); no lock; cons reported as 2 */
#define CSDR_DIGITAL_TABLE 9         /* ModemAPSK / ModemSQAM / ModemST: a caller-supplied constellation; only through csdr_bank_configure_table_slot */

typedef struct csdr_digital_params {
    int32_t kind;              /* CSDR_DIGITAL_* (the reference class) */
    int32_t cons;              /* PSK / DPSK / ASK: 2..256, QAM: 4..256, a power of two ("cons" setting); 0 = the reference default (2; QAM 4) */
    int32_t bps;               /* FSK bits per symbol ("bps"; 0 = 1) */
    int32_t sps;               /* FSK symbols per second ("sps"; 0 = 9600).  GMSK: SAMPLES per symbol ("sps", 2..512; 0 = 4) -- not FSK's meaning */
    float   bw;                /* FSK signal bandwidth as a fraction of the modem rate ("bw"; 0 = 0.45).  GMSK: the BT product ("ebf"; 0 = 0.3) */
    int32_t fdelay;            /* GMSK filter delay in symbols ("fdelay", 1..128; 0 = 3); else 0 */
    int32_t reserved[2];       /* 0 */
} csdr_digital_params;

/* per (digital slot, block) of the last execute */
typedef struct csdr_digital_result {
    int32_t n_symbols;         /* decisions of this block */
    int32_t symbol_offset;     /* where they start in csdr_bank_fetch_symbols' output */
    int32_t lock;              /* updateDemodulatorLock after the block (ModemDigital.cpp:51-53): evm <= the modem's sensitivity; FSK: 0 */
    float   evm;               /* modemcf_get_demodulator_evm after the block: |x_hat - r| of the last decided sample (a block without samples
                                  repeats the previous value); FSK: 0 */
    int32_t carry;             /* FSK: samples held for the next symbol after the block (kit->inputBuffer.size()); GMSK: the same count, which can
                                  grow far above sps (ModemGMSK never reads those samples); else 0 */
    int32_t cons;              /* the constellation size the block was decided with (FSK: 2^bps; BPSK / QPSK / OOK: 2, 4, 2) */
    int32_t reserved[2];
} csdr_digital_result;

/* state of one modem object for csdr_digital_run (zero = freshly created) */
#define CSDR_DIGITAL_MAX_CARRY 2048
typedef struct csdr_digital_state {
    float   r[2], x_hat[2];    /* last demodulated sample and its re-modulated decision (what the EVM compares) */
    float   phi;               /* DPSK: phase of the previous input sample */
    int32_t n_carry;           /* FSK: samples carried (< k) */
    int32_t reserved[2];
    float   carry[2 * CSDR_DIGITAL_MAX_CARRY];   /* FSK: the carried samples, interleaved complex */
} csdr_digital_state;

/* (Re)build slot `slot` as a digital modem: p->modem must be CSDR_MODEM_DIGITAL; p->bandwidth is the modem rate before checkSampleRate
 * (ModemDigital.cpp:21-26: at least 500 Hz; ModemFSK.cpp:19-28).  Every constellation of the kind starts fresh.  CSDR_EUNSUPPORTED for settings
 * the reference cannot build: a cons outside its list, FSK with k = rate / sps outside [2, 2048] or bw outside (0, 0.5) (fskdem_create returns
 * no object), or tones that share a transform bin (fskdem_create reports that and goes on; bps above 16 always does). */
int  csdr_bank_configure_digital_slot(csdr_bank *bank, int slot, const csdr_demod_params *p, const csdr_digital_params *d, const csdr_post *post);
/* writeSetting("cons") (updateDemodulatorCons): switch to constellation `cons` from the next execute on.  The front-end is not reset, and every
 * constellation keeps its own state (ModemPSK and alike create all of them up front): switching back resumes where that one stopped. */
int  csdr_bank_set_digital_cons(csdr_bank *bank, int slot, int cons);
/* per-block results of the last execute (synchronises) */
int  csdr_bank_fetch_digital_results(csdr_bank *bank, int slot, csdr_digital_result *out, int cap_blocks, int *n_blocks);
/* the symbols of the last execute, all blocks in order (synchronises) */
int  csdr_bank_fetch_symbols(csdr_bank *bank, int slot, uint32_t *host_out, int cap, int *n);
/* The decision kernel alone on n caller-supplied samples at the modem rate `sample_rate` (FSK: k = sample_rate / sps), one modem object whose
 * state is *state (read, then updated); for parity checks on identical input.  Symbols go to sym_host (*n_symbols of them: n for a
 * constellation, whole symbols for FSK), *evm_last is the object's EVM afterwards (FSK: 0). */
int  csdr_digital_run(csdr_ctx *ctx, const csdr_digital_params *d, int64_t sample_rate, const float *iq_host, int n, csdr_digital_state *state,
                      uint32_t *sym_host, int cap_symbols, int *n_symbols, float *evm_last);

/* GMSK object state for csdr_gmsk_run (zero = freshly created); the filter window travels beside it in a caller-owned history of
 * 2 sps fdelay floats (the last phase differences pushed, oldest first; zeros when fresh) */
typedef struct csdr_gmsk_state {
    float   x_prime[2];        /* the last sample demodulated */
    int32_t reserved[2];
} csdr_gmsk_state;

/* The GMSK kernels alone on n caller-supplied samples (a multiple of sps): n / sps consecutive gmskdem_demodulate calls of one object whose state
 * is *state and history (read, then updated); for parity checks on identical input.  Decisions go to sym_host, the receive filter's outputs they
 * were taken from to soft_host (may be NULL); *n_symbols = n / sps.  CSDR_EUNSUPPORTED where csdr_bank_configure_digital_slot refuses. */
int  csdr_gmsk_run(csdr_ctx *ctx, const csdr_digital_params *d, const float *iq_host, int n, csdr_gmsk_state *state, float *history,
                   uint32_t *sym_host, float *soft_host, int cap_symbols, int *n_symbols);

#ifdef __cplusplus
#define CSDR_STATIC_ASSERT(c, m) static_assert(c, m)
#else
#define CSDR_STATIC_ASSERT(c, m) _Static_assert(c, m)
#endif
/* the digital lab's structures keep their layout */
CSDR_STATIC_ASSERT(sizeof(csdr_digital_params) == 32 && offsetof(csdr_digital_params, bw) == 16 && offsetof(csdr_digital_params, fdelay) == 20,
                   "csdr_digital_params layout");
CSDR_STATIC_ASSERT(sizeof(csdr_digital_result) == 32 && offsetof(csdr_digital_result, carry) == 16, "csdr_digital_result layout");
CSDR_STATIC_ASSERT(sizeof(csdr_digital_state) == 32 + 8 * CSDR_DIGITAL_MAX_CARRY && offsetof(csdr_digital_state, carry) == 32, "csdr_digital_state layout");
CSDR_STATIC_ASSERT(sizeof(csdr_gmsk_state) == 16, "csdr_gmsk_state layout");

/* ---- table-driven constellations (ModemAPSK.cpp, ModemSQAM.cpp, ModemST.cpp; liquid's modemcf_create_arbitrary and its APSK objects)
 * The points are caller data, numbered by symbol: what modemcf_modulate returns for s = 0 .. n_points - 1.  Three decision rules, per sample x:
 *   CSDR_TABLE_NEAREST  modemcf_demodulate_arb (the arb family and V.29): the FIRST s that minimises |x - points[s]|^2, every operation rounded
 *                       in float32.
 *   CSDR_TABLE_QUADRANT modemcf_demodulate_sqam32 / _sqam128: q = 2 (re < 0) + (im < 0); x is folded into the first quadrant by those signs
 *                       (re and im negated where negative: exact); the first nearest point s' among the first n_points / 4, as above; the symbol is
 *                       s' + q n_points / 4.  The table must have that structure: points[s' + n_points / 4] = conj(points[s']), [s' + 2 n_points / 4] =
 *                       -conj, [s' + 3 n_points / 4] = -points[s'], bit for bit.  Off the axes this decides as NEAREST does, except for samples so
 *                       small that x - points[s] rounds to -points[s] in float32: there NEAREST sees four equal distances and takes the first, the
 *                       fold still follows the signs -- and such samples do occur (a front-end's first outputs after a reset).
 *   CSDR_TABLE_RINGS    modemcf_demodulate_apsk: rad = sqrtf(x.re^2 + x.im^2); the ring l is the first with rad < ring_slicer[l], else the last;
 *                       theta = atan2f(im, re), plus 2 pi when negative; j = roundf((theta - ring_phase[l]) / (float)(2 pi / ring_size[l])) reduced by
 *                       the true modulo ring_size[l]; the symbol is the s with ring_map[s] = ring_size[0] + .. + ring_size[l - 1] + j.
 *                       (liquid casts a negative j to unsigned before its modulo; with a ring phase of 0 -- every table of liquid -- theta is never
 *                       negative and that path never runs, so a table with other phases has no reference behaviour to differ from.)
 * Either way x_hat = points[s], the EVM is |x_hat - x| of the block's last decided sample and the lock is evm <= sensitivity, as for the
 * other constellations. */
#define CSDR_TABLE_NEAREST    0
#define CSDR_TABLE_RINGS      1
#define CSDR_TABLE_QUADRANT   2
#define CSDR_TABLE_MAX_POINTS 256
#define CSDR_TABLE_MAX_RINGS  8
#define CSDR_TABLE_MAX_TABLES 8
typedef struct csdr_constellation {
    int32_t rule;              /* CSDR_TABLE_* */
    int32_t n_points;          /* a power of two in 2 .. 256 (QUADRANT: 4 .. 256) */
    float   sensitivity;       /* updateDemodulatorLock's second argument; 0 = 0.005 (what ModemAPSK, ModemSQAM and ModemST pass) */
    int32_t n_rings;           /* RINGS: 1 .. 8; else 0 */
    float   points[2 * CSDR_TABLE_MAX_POINTS];     /* interleaved complex, by symbol */
    int32_t ring_size[CSDR_TABLE_MAX_RINGS];       /* RINGS: points on ring l, inner ring first; they sum to n_points */
    float   ring_radius[CSDR_TABLE_MAX_RINGS];
    float   ring_phase[CSDR_TABLE_MAX_RINGS];      /* argument of the ring's point of index 0 */
    float   ring_slicer[CSDR_TABLE_MAX_RINGS];     /* [n_rings - 1] used: the radius that parts ring l from ring l + 1 */
    uint8_t ring_map[CSDR_TABLE_MAX_POINTS];       /* symbol -> ring-ordered index (rings in order, each ring's points by phase index) */
} csdr_constellation;
CSDR_STATIC_ASSERT(sizeof(csdr_constellation) == 2448 && offsetof(csdr_constellation, points) == 16 && offsetof(csdr_constellation, ring_size) == 2064 &&
                   offsetof(csdr_constellation, ring_radius) == 2096 && offsetof(csdr_constellation, ring_phase) == 2128 &&
                   offsetof(csdr_constellation, ring_slicer) == 2160 && offsetof(csdr_constellation, ring_map) == 2192, "csdr_constellation layout");
/* The ring description of an APSK constellation from its points alone (host only; no liquid table is needed): *out gets rule = CSDR_TABLE_RINGS,
 * sensitivity 0, the points and the rings.  The points are sorted by radius; points whose radii exceed that of the ring's innermost point by at most
 * 1e-4 of the largest radius form one ring; rings are ordered by radius.  A ring of radius below that tolerance holds one point and gets phase 0; any other ring's phase is its
 * smallest argument in [0, 2 pi) (an argument within 1e-6 below 0 counts as 0), a point's index in its ring is round((arg - phase) / (2 pi / p)) mod p,
 * every index occurs once and every point lies within 1e-4 rad of its index's place; slicers are the float midpoints of neighbouring radii.
 * CSDR_EINVAL for anything else: a size that is not a power of two in 2 .. 256, duplicate points, more than 8 rings, rings that are not concentric
 * and evenly spaced. */
int  csdr_design_rings(const float *points, int n_points, csdr_constellation *out);
/* (Re)build slot `slot` as a table-driven digital modem: p->modem must be CSDR_MODEM_DIGITAL, the rate rule is ModemDigital.cpp:21-26 (at least
 * 500 Hz).  `tables`: 1 .. 8 constellations with distinct n_points -- the reference classes' per-"cons" modem objects, all created up front, each
 * with its own r / x_hat state (kept in two copies, as the other constellations' records) -- of which the first is active.  CSDR_EINVAL for a
 * table that is not well formed (rule, sizes, non-finite values, a ring_map that is no permutation, slicers that do not ascend).
 * csdr_bank_set_digital_cons(bank, slot, n_points) switches the active table and resets nothing (CSDR_EUNSUPPORTED: no table of that size);
 * csdr_bank_fetch_digital_results (cons = the deciding table's n_points) and csdr_bank_fetch_symbols serve these slots as any constellation. */
int  csdr_bank_configure_table_slot(csdr_bank *bank, int slot, const csdr_demod_params *p, const csdr_constellation *tables, int n_tables,
                                    const csdr_post *post);
/* The table kernel alone on n caller-supplied samples, one modem object whose state is *state (r and x_hat: read, then updated); for parity
 * checks on identical input, the counterpart of csdr_digital_run.  *n_symbols = n; *evm_last is the object's EVM afterwards. */
int  csdr_table_run(csdr_ctx *ctx, const csdr_constellation *table, const float *iq_host, int n, csdr_digital_state *state,
                    uint32_t *sym_host, int cap_symbols, int *n_symbols, float *evm_last);

/* ------------------------------------------------------------------ SpectrumVisualProcessor (src/process/SpectrumVisualProcessor.cpp)
 * replaces: setup :140-178 (fft_create_plan(2*fftSize, FORWARD)), process :212-637 full-span view:
 * frame selection :387-421, fft_execute :439, magnitude + fftshift :441-452, double EMA + min/max :494-530,
 * floor/ceil EMAs :518-530, display resample + log10 scaling :532-576. */
#define CSDR_SPEC_FIRST_FRAME 0  /* reference cadence: only the first 2*fftSize samples of each block (:387-397) */
#define CSDR_SPEC_CONTIGUOUS  1  /* every sample belongs to one non-overlapping 2*fftSize frame */
#define CSDR_SPEC_LINES       2  /* every block is one input shorter than 2*fftSize (the fftSize-sample lines FFTDataDistributor
                                  * emits, FFTDataDistributor.cpp:112-131): the first one primes fftLastData, each later one is
                                  * appended to the previous FFT input shifted left by its length (:399-421) -> one frame each */

int  csdr_spec_create(csdr_ctx *ctx, csdr_spec **out);
void csdr_spec_destroy(csdr_spec *spec);
int  csdr_spec_setup(csdr_spec *spec, int fft_size, int max_frames);      /* setup(fftSize_in): a power of two up to 2^21, or any other size up to 2^20 (setFFTSize :180-190 takes any) */
int  csdr_spec_set_average_rate(csdr_spec *spec, float rate);             /* setFFTAverageRate, default 0.65 (:36) */
int  csdr_spec_set_scale_factor(csdr_spec *spec, float sf);               /* setScaleFactor, default 1 */
/* setPeakHold (:115-125): enabling starts a one-input countdown to the reset of fft_result_peak / fft_ceil_peak /
 * fft_floor_peak (:264-273), enabling again while enabled restarts it at PEAK_RESET_COUNT = 30 inputs; frames after the
 * reset carry spectrum_hold_points and are scaled by the held ceiling / floor (:506-510, :523-541). */
int  csdr_spec_set_peak_hold(csdr_spec *spec, int enabled);
int  csdr_spec_get_peak_hold(const csdr_spec *spec);
/* setHideDC (:204-209) and the frequencies its bin arithmetic uses (:578-623): setCenterFrequency, setBandwidth, and
 * iqData->frequency of the inputs that follow.  Applied to the points as they are fetched. */
int  csdr_spec_set_hide_dc(csdr_spec *spec, int enabled);
int  csdr_spec_set_center_frequency(csdr_spec *spec, int64_t center_freq);
int  csdr_spec_set_bandwidth(csdr_spec *spec, int64_t bandwidth);
int  csdr_spec_set_input_frequency(csdr_spec *spec, int64_t frequency);
/* Zoomed view: setView(bView[, centerFreq, bandwidth]) :64-72 with setCenterFrequency / setBandwidth above.  While set, every
 * csdr_spec_process call is ONE process() input (n_blocks == 1; `mode` is ignored) taken through :283-386: the sample rate
 * is halved while half of it still covers `bandwidth`, the first fftSizeInternal / ratio samples are shifted by
 * centerFreq - input frequency (nco_crcf) and resampled (msresamp_crcf_create(ratio, 60)), the averagers follow retunes and
 * zoom steps (:316-331, :454-492), and the display walks bandwidth / resampleBw bins per point (:532-560).
 * csdr_spec_set_input_rate gives iqData->sampleRate of the inputs that follow (it also stands in for the application
 * sample rate of the range test :308). */
int  csdr_spec_set_view(csdr_spec *spec, int is_view);
int  csdr_spec_get_view(const csdr_spec *spec);
int  csdr_spec_set_input_rate(csdr_spec *spec, int64_t sample_rate);
int  csdr_spec_desired_input_size(const csdr_spec *spec);                 /* getDesiredInputSize :133-137 */
/* Run the spectrum path over n_blocks x block_len samples; frames are taken per `mode`.  Every frame updates the
 * averagers in order, exactly as one process() call per frame would. */
int  csdr_spec_process(csdr_spec *spec, const float *iq, int iq_is_dev, int n_blocks, int block_len, int mode);
int  csdr_spec_frames(const csdr_spec *spec);                             /* frames produced by the last process */
/* SpectrumVisualData of frame `frame` of the last process: spectrum_points[2*fftSize] = (x, y) pairs,
 * fft_ceiling, fft_floor (SpectrumVisualProcessor.h:14-23; :626-627). */
int  csdr_spec_fetch(csdr_spec *spec, int frame, float *points_host, int cap_floats, double *fft_ceiling, double *fft_floor);
/* spectrum_hold_points[2*fftSize] of that frame; *n_floats = 0 when the frame carries none (peak hold off or not reset yet) */
int  csdr_spec_fetch_hold(csdr_spec *spec, int frame, float *hold_host, int cap_floats, int *n_floats);
/* raw forward FFT of one 2*fftSize frame (K13 alone), for parity tests against fft_execute */
int  csdr_spec_fft_only(csdr_spec *spec, const float *iq_host, float *out_host);

/* ------------------------------------------------------------------ ScopeVisualProcessor (src/process/ScopeVisualProcessor.cpp)
 * replaces: setup :24-35 (fft_create_plan(fftSize)), process :45-217 -- waveform normalisation by max(1, peak) in the modes Y / 2Y / XY
 * (:64-117), the audio spectrum: zero-padded real input (stereo: left + right) -> fft_execute :163 -> |X| in double -> the two averagers
 * (the second one sees the UPDATED first one, :176-177) -> double extrema -> floor / ceil trackers :186-190 -> log10 scaling :202-206,
 * outSize = floor(fftSize/2 * sampleRate / inputRate) :194-200.  Every frame is one AudioThreadInput; frames of a call are processed in
 * order through ONE state, exactly as consecutive process() calls. */
typedef struct csdr_scope_frame {
    const float *data;          /* n floats; host memory, or device memory when csdr_scope_process(..., data_is_dev = 1) */
    const int32_t *n_dev;       /* device frames only: NULL, or a device int that bounds n (csdr_bank_scope_frame sets it) */
    int32_t n;                  /* AudioThreadInput::data.size() */
    int32_t channels;           /* 1 | 2 */
    int32_t type;               /* AudioThreadInput::type: 0 -> SCOPE_MODE_Y, 1 -> SCOPE_MODE_2Y, 2 -> SCOPE_MODE_XY (:84, :95, :104) */
    int32_t sample_rate, input_rate;
    int32_t layout;             /* 0: data is in AudioThreadInput order.  1 / 2: data is n/2 interleaved pairs (a, b) as a stereo demodulator
                                 * wrote them; the frame the scope sees is  1: [a.. | b..] * scale   2: [b.. | a..] * scale  (the re-packing
                                 * of DemodulatorThread.cpp:269-291 done while the tap is read, in place in HBM) */
    float   scale;
} csdr_scope_frame;
typedef struct csdr_scope_info {   /* ScopeRenderData (ScopeVisualProcessor.h:10-21) without the points */
    int32_t mode, spectrum, channels, input_rate, sample_rate, fft_size, n_floats, reserved;
    double  fft_floor, fft_ceil;
} csdr_scope_info;
int  csdr_scope_create(csdr_ctx *ctx, csdr_scope **out);
void csdr_scope_destroy(csdr_scope *scope);
int  csdr_scope_setup(csdr_scope *scope, int fft_size, int max_frames, int max_samples);   /* setup(fftSize_in); fft_size <= 4096 */
int  csdr_scope_set_enabled(csdr_scope *scope, int scope_enabled, int spectrum_enabled);  /* :37-43 */
int  csdr_scope_set_max_scope_samples(csdr_scope *scope, int n);                            /* maxScopeSamples, default DEFAULT_DMOD_FFT_SIZE = 1024 (:13) */
int  csdr_scope_set_average_rate(csdr_scope *scope, float rate);                            /* fft_average_rate, default 0.65 (:10) */
int  csdr_scope_process(csdr_scope *scope, const csdr_scope_frame *frames, int n_frames, int data_is_dev);
int  csdr_scope_frames(const csdr_scope *scope);
/* item of frame `frame` of the last process: which = 0 the waveform, 1 the spectrum; info->n_floats == 0 when it was not produced */
int  csdr_scope_fetch(csdr_scope *scope, int frame, int which, float *points_host, int cap_floats, csdr_scope_info *info);
/* the audio-scope tap of a demodulator for the LAST block of the bank's last execute (DemodulatorThread.cpp:240-316), as a frame
 * whose data lies in HBM (pass it to csdr_scope_process with data_is_dev = 1); out->n == 0: nothing to show */
int  csdr_bank_scope_frame(csdr_bank *bank, int slot, csdr_scope_frame *out);

/* ------------------------------------------------------------------ WaterfallPanel (src/panel/WaterfallPanel.cpp, src/util/Gradient.cpp)
 * replaces: setup :13-24, setPoints :39-49, step :51-83, update :85-159, refreshTheme :26-37 with Gradient::generate (Gradient.cpp:37-85), and
 * the unscaled picture of drawPanelContents :161-219; fed as WaterfallCanvas::processInputQueue feeds it (src/visual/WaterfallCanvas.cpp:89-126).
 * The display points of a spectrum stay in HBM from csdr_spec_process to the coloured picture, and to the picture scaled and filtered to a viewport
 * ("Waterfall viewport" below).
 * All work of a waterfall runs on a stream of its own; the calls that return data to the host synchronise it.
 *
 * 1. Quantiser (:64-72).  wv = v < 0 ? 0 : (v > 0.99 ? 0.99 : v), stored to a float, then (unsigned char)floor(wv * 255.0).  The comparison with
 *    0.99 is made in double, the clamp value becomes (float)0.99: the highest index is 252, for 0.99f, 1.0, +inf and everything between.  -0.0 and
 *    every negative give 0.  A NaN has no defined result in the reference (the conversion is undefined); THE LIBRARY'S OWN DEFINITION is 0.
 * 2. Lines and halves.  half = fft_size / 2 (integer division); byte i of half j comes from point j * half + i (:65-67); with an odd fft_size the
 *    last point is not drawn, as in the reference.  A line of 2 * fft_size floats is the (x, y) pairs of SpectrumVisualData and its y values are
 *    used (:40-45); a line of fft_size floats is used as it stands (:47); any other length -- or points == NULL -- leaves the previous points in
 *    place and the step repeats them, which is what WaterfallCanvas.cpp:106-109 does with a frame of the wrong size.  After a setup the points
 *    are those of before (:18-20: resized to fft_size, new ones zero).
 * 3. Texture life cycle.  setup clears lines_buffered and marks the textures uninitialised (:16, :22-23).  Steps before the first update after a
 *    setup are dropped (:60-62; *taken = 0; their points are still kept, setPoints does not depend on the textures).  The first update after a
 *    setup and at least one step call (:88-90) creates both rings zero-filled with waterfall_ofs = lines - 1 (:92-130).  A call that would make
 *    more than max_pending lines wait for an update is refused as a whole with CSDR_ERANGE: nothing is taken, nothing changes.
 * 4. update is :132-158 literally: the pending lines are reversed (newest first) and written in runs of min(lines_buffered, waterfall_ofs[0]) rows
 *    at rows [ofs - run, ofs); after each run ofs -= run, and an offset that reaches 0 becomes `lines`.  Two consequences are the reference's and
 *    are kept: row lines - 1 is not written during the first turn of the ring, and when one update crosses the wrap the older remainder lands
 *    above the newer run.  lines = 7: step A, B, C, update -> rows 3, 4, 5 hold C, B, A, ofs = 3; step D, E, F, G, H, update -> rows 0 .. 6 hold
 *    H, G, F, C, B, E, D, ofs = 5.  (lines >= 2: with one line the reference's loop never ends.)
 * 5. Gradient (Gradient.cpp:37-85).  n colour stops -> len entries: chunk_size = len / (n - 1), the last chunk takes the remainder; per entry
 *    idx = (float)i / (float)chunk_size, then c1 + (c2 - c1) * idx in float with each operation rounded on its own, then a clamp to [0, 1].
 *    2 <= n_colors <= len + 1, anything else is CSDR_EINVAL (chunk_size 0 divides by zero in the reference).  The stops are CALLER DATA, r, g, b
 *    interleaved: the library carries no theme of the reference; the application passes what it reads from its own ColorTheme.  GL's conversion of
 *    the mapped float to a texel is implementation-defined; THE LIBRARY'S OWN DEFINITION is (uint8)(c * 255.0f + 0.5f) per channel (product and
 *    sum rounded one by one), alpha 255, computed once per set_gradient on the host: the device table is 256 x RGBA8 (bytes r, g, b, a).  Before
 *    any set_gradient the table is the grey ramp i -> (i, i, i, 255).  The table outlives a setup.
 * 6. fetch_rgba is the picture drawPanelContents shows, unscaled (:186-213: the texture coordinate t runs from waterfall_ofs / lines under
 *    GL_REPEAT): image row r is ring row (ofs + first_row + r) mod lines of half 0 followed by the same row of half 1, 2 * half pixels of 4 bytes,
 *    each coloured through the table; first_row >= 0, n_rows >= 1, first_row + n_rows <= lines.  out_u8 == NULL leaves the picture on the device;
 *    csdr_waterfall_device_rgba returns the last rendered picture ([n_rows][2 * half] RGBA8, dense) and makes the context's boundary stream wait
 *    for it, so a consumer enqueued there reads the finished picture.  It stays valid until the next fetch_rgba or setup.
 * 7. step_spec takes frames frame0 .. frame0 + n_frames - 1 of the spectrum's last csdr_spec_process straight from its point buffer in HBM, ordered
 *    behind the averaging lane's work by an event (no host synchronisation; the spectrum's next process in turn waits for these reads).  With
 *    csdr_spec_set_hide_dc on it applies the DC-spike overwrite exactly as csdr_spec_fetch does.  A spectrum whose fftSize is not the waterfall's
 *    fft_size is a frame of the wrong size (item 2).  What csdr_spec_fetch returns is not changed by it. */
int  csdr_waterfall_create(csdr_ctx *ctx, csdr_waterfall **out);
void csdr_waterfall_destroy(csdr_waterfall *wf);
int  csdr_waterfall_setup(csdr_waterfall *wf, int fft_size, int lines, int max_pending);     /* setup(fft_size_in, num_waterfall_lines_in); fft_size 2 .. 2^21 */
/* Gradient::generate(len): r, g, b receive len floats each; host only, needs no device */
int  csdr_design_gradient(const float *rgb_stops, int n_colors, int len, float *r, float *g, float *b);
int  csdr_waterfall_set_gradient(csdr_waterfall *wf, const float *rgb_stops, int n_colors);  /* refreshTheme: generate(256) -> the RGBA8 table in HBM */
/* setPoints + step for each of n_lines lines of n_floats_per_line floats (host memory, or device memory produced on the boundary stream when
 * is_dev != 0); *taken (may be NULL) = the lines that went into the pending buffer.  Host lines are copied with hipMemcpyAsync: from page-locked
 * memory the copy may still be in flight when the call returns, so such a buffer stays unchanged until the next synchronising call on this object
 * (csdr_waterfall_fetch_index, csdr_waterfall_fetch_rgba with a host buffer); device lines stay unchanged until then as well */
int  csdr_waterfall_step(csdr_waterfall *wf, const float *points, int is_dev, int n_floats_per_line, int n_lines, int *taken);
int  csdr_waterfall_step_spec(csdr_waterfall *wf, csdr_spec *spec, int frame0, int n_frames, int *taken);
int  csdr_waterfall_update(csdr_waterfall *wf);                                              /* WaterfallPanel::update */
int  csdr_waterfall_lines_buffered(const csdr_waterfall *wf);
int  csdr_waterfall_offset(const csdr_waterfall *wf, int half);                              /* waterfall_ofs[half]; -1 while there are no textures */
/* one ring texture: lines x (fft_size / 2) bytes, rows as GL holds them (synchronises) */
int  csdr_waterfall_fetch_index(csdr_waterfall *wf, int half, uint8_t *out_u8, int64_t cap);
int  csdr_waterfall_fetch_rgba(csdr_waterfall *wf, int first_row, int n_rows, uint8_t *out_u8, int64_t cap);
int  csdr_waterfall_device_rgba(csdr_waterfall *wf, const uint8_t **dev);

/* ------------------------------------------------------------------ Waterfall viewport (src/panel/WaterfallPanel.cpp:161-219)
 * replaces: the two textured quads drawPanelContents draws with GL_LINEAR / GL_REPEAT (:117-120) into whatever viewport the canvas has -- a
 * width x height RGBA8 picture of the ring, rendered in HBM from the two ring textures and the colour table, so that a headless consumer pulls
 * W * H * 4 bytes over the link and not the ring at texture resolution.  half = fft_size / 2, L = lines, ofs = waterfall_ofs; image row 0 is the
 * top, as in fetch_rgba.  All coordinate arithmetic is exact integer arithmetic on the host (int64); the device reads tables of csdr_view_tap.
 *
 * 1. Limits.  fft_size >= 4, 2 <= width <= 16384, 1 <= height <= 16384, mode one of the two below; anything else is CSDR_EINVAL.  Before the
 *    textures exist the call returns what csdr_waterfall_fetch_rgba returns then (CSDR_ESTATE); a host buffer that is too small is CSDR_ERANGE.
 *    A refusal renders nothing and changes nothing.
 * 2. Which half a pixel shows.  The reference's quads meet with a half-pixel overlap (:185, :195, :206) and the second is drawn over the first; GL
 *    leaves a pixel centre that lies exactly on an edge to the implementation.  THE LIBRARY'S OWN DEFINITION: pixel column px shows half 1 iff
 *    2 px + 2 > W, otherwise half 0 -- W / 2 pixels each for an even W, the middle pixel to half 1 for an odd one.
 * 3. CSDR_WF_VIEW_LINEAR is the reference's picture: the texture coordinates are affine over each quad and sampled at pixel centres.
 *    Columns: num = 2 px + 1 (half 0) or 2 px + 2 - W (half 1); u = 0.5 + (half - 2) num / (W + 1), which is :186, :192-198 and :205-211 with
 *    half_texel = 1 / half -- the reference's bias trims one texel at each end of a half, and that is kept.  i0 = floor(u), i1 = i0 + 1,
 *    alpha = u - i0; i0 lies in [0, half - 2], so GL_REPEAT never acts horizontally.
 *    Rows: n = L (2 py + 1) - H, q = floor(n / 2H) in [-1, L - 1], beta = (n mod 2H) / 2H; ring rows j0 = (ofs + q + L) mod L and
 *    j1 = (j0 + 1) mod L.  Under GL_REPEAT with H > L the top and bottom pixel rows blend the newest line with the oldest: the reference's
 *    behaviour, kept.  With H = L every beta is 0 and row py is ring row (ofs + py) mod L, as in fetch_rgba.
 *    alpha and beta are (float)((double)numerator / (double)denominator) of those integers.
 *    The texture holds colours, not indices (:122, GL_RGB from GL_COLOR_INDEX), so table colours are blended, per channel, from the table's bytes
 *    taken as floats: top = c00 + alpha (c10 - c00), bot = c01 + alpha (c11 - c01), m = top + beta (bot - top), channel = (uint8)(m + 0.5f),
 *    every operation rounded to float32 on its own; alpha channel 255.  (cXY: texel iX of ring row jY.)  GL's filter precision is
 *    implementation-defined: this is THE LIBRARY'S OWN DEFINITION, in the sense of item 5 of the block above.
 * 4. CSDR_WF_VIEW_PEAK is THE LIBRARY'S OWN MODE, not the reference's: GL_LINEAR without mipmaps samples 2 x 2 texels per pixel, which at 34
 *    points per pixel skips 94 % of the bins.  Here no bin and no line is lost.  Half h owns n_h pixels by item 2; its k-th pixel shows texels
 *    [k half div n_h, (k + 1) half div n_h), image row py shows scrolled rows [py L div H, (py + 1) L div H), an empty range becomes its single
 *    first element; scrolled row r is ring row (ofs + r) mod L.  The pixel is the table colour of the MAXIMUM INDEX BYTE over that rectangle.
 *    With W = 2 half and H = L the picture equals csdr_waterfall_fetch_rgba(0, L) byte for byte; with n_h <= half and H <= L every texel of the
 *    ring is read exactly once.
 * 5. Tap tables.  csdr_design_view_columns / csdr_design_view_rows are that arithmetic (host only, no device needed): LINEAR gives first = i0 or
 *    q, count = 2, frac = alpha or beta; PEAK gives the range's start and length and frac = 0; `half` is the column's half (0 for rows).  They
 *    do not depend on ofs: a waterfall keeps its tables on the device per (fft_size, lines, width, height, mode) and rebuilds them only when one
 *    of those changes.
 * 6. render_view renders on the waterfall's stream into a buffer of its own ([height][width] RGBA8, dense): what csdr_waterfall_device_rgba promises
 *    about the last fetch_rgba picture still holds.  out_u8 == NULL leaves the picture on the device; otherwise width * height * 4 bytes are copied
 *    to the host and the stream is synchronised.  csdr_waterfall_device_view returns the last rendered view and its size and makes the context's
 *    boundary stream wait for it; it stays valid until the next render_view or setup. */
#define CSDR_WF_VIEW_LINEAR 0
#define CSDR_WF_VIEW_PEAK   1
typedef struct csdr_view_tap {
    int32_t first, count;      /* LINEAR: i0 or q, 2; PEAK: start and length of the range */
    float   frac;              /* LINEAR: alpha or beta; PEAK: 0 */
    int32_t half;              /* columns: the half the pixel shows; rows: 0 */
} csdr_view_tap;
CSDR_STATIC_ASSERT(sizeof(csdr_view_tap) == 16 && offsetof(csdr_view_tap, frac) == 8 && offsetof(csdr_view_tap, half) == 12, "csdr_view_tap layout");
int  csdr_design_view_columns(int fft_size, int width, int mode, csdr_view_tap *taps);       /* taps[width] */
int  csdr_design_view_rows(int lines, int height, int mode, csdr_view_tap *taps);            /* taps[height]; lines 2 .. 2^20 */
int  csdr_waterfall_render_view(csdr_waterfall *wf, int width, int height, int mode, uint8_t *out_u8, int64_t cap);
int  csdr_waterfall_device_view(csdr_waterfall *wf, const uint8_t **dev, int *width, int *height);

/* ------------------------------------------------------------------ FFTDataDistributor (src/process/FFTDataDistributor.cpp)
 * replaces: the ctor's defaults :11, setFFTSize :15-18, setLinesPerSecond :20-22 and, per csdr_distrib_push, ONE popped input of process() :41-143
 * statement for statement -- the reset on a change of rate or frequency :42-53, the growth on an fft change alone :56-59, compaction and overflow
 * :66-76, the append :79-80, the pacing arithmetic :89-96, "move along" :101-104, the accumulate / emit / wrap loop :106-129, the offset clamp
 * :133-141.  All of that is host integer and double arithmetic in the reference's order of operations; the samples are only copied, and they are
 * copied inside HBM: the block is read where the ingest (or the caller) put it, the lines land in a batch the spectrum reads in place
 * (csdr_spec_process_distrib), and nothing crosses the link.
 *
 * 1. The buffer.  After every input fewer than fft_size samples stay buffered, so the reference's 0.25 s buffer is not kept: the device holds the
 *    carried samples only (bufferedItems of them; after fft_size shrank there can be more than the new fft_size -- up to the largest fft_size used
 *    so far, minus one), and a push works on the virtual stream carry ++ block.  bufferMax and bufferOffset are kept as the integers they are in
 *    the reference, because they decide the overflow rule: when bufferOffset + bufferedItems + n_samples > bufferMax the offset returns to 0, and
 *    if bufferedItems + n_samples still exceeds bufferMax the LAST n_samples - (bufferMax - bufferedItems) incoming samples are dropped (:66-76).
 * 2. A line is fft_size consecutive samples of that stream starting at a multiple of fft_size; which of them go out is the accumulator's decision
 *    (:106-129).  The reference pushes lines to its output queues without blocking and loses what does not fit (:121); here every emitted line
 *    is in the batch, and a push that would emit more than max_lines lines is refused as a whole.
 * 3. Refusals: CSDR_EINVAL for fft_size < 1, lines per second < 0, sample_rate <= 0, n_samples < 0 (or a null block with n_samples > 0, or a
 *    device block that is not 8-byte aligned); CSDR_ERANGE for a push that would emit more than max_lines lines.  A refusal enqueues nothing and
 *    leaves the state, the carried samples and both batches as they were.
 * 4. Two batches alternate: the pointer csdr_distrib_lines returns holds the lines of the last push ([n_lines][line_len] complex samples, dense)
 *    and stays valid, with its contents, until the second push after it.
 * 5. Ordering.  The distributor's copies run on a stream of its own.  A device block is ordered behind its producer as csdr_spec_process orders a
 *    device input (work enqueued on the boundary stream, the ingest's transfer), and its reads are joined to the spectrum's FFT lane, so an
 *    ingest ring recycles the block behind them.  csdr_spec_process_distrib makes the spectrum wait for the copy by an event and leaves one the
 *    distributor waits for before it rewrites that batch: no host synchronisation between push, spectrum and csdr_waterfall_step_spec.  (The table
 *    of line starts is uploaded from page-locked memory that a push reuses two pushes later; it first waits for that earlier copy, long done.)
 *    A host block (iq_is_dev = 0; for callers without an ingest) is staged as a whole with hipMemcpyAsync: from page-locked memory the copy may
 *    still be in flight when the call returns, so such a block stays unchanged until the next synchronising call on this object (the fetches). */
typedef struct csdr_distrib_state {
    double  line_rate_accum;   /* lineRateAccum */
    int64_t buffered_items;    /* bufferedItems */
    int64_t buffer_offset;     /* bufferOffset */
    int64_t buffer_max;        /* bufferMax */
    int64_t dropped;           /* incoming samples the last push dropped (:71-75) */
    int32_t n_lines;           /* lines the last push emitted */
    int32_t line_len;          /* their length: the fft_size that push read */
} csdr_distrib_state;
CSDR_STATIC_ASSERT(sizeof(csdr_distrib_state) == 48 && offsetof(csdr_distrib_state, n_lines) == 40, "csdr_distrib_state layout");
int  csdr_distrib_create(csdr_ctx *ctx, int max_lines, csdr_distrib **out);                   /* ctor :11: fft_size 2048, 30 lines per second */
void csdr_distrib_destroy(csdr_distrib *d);
int  csdr_distrib_set_fft_size(csdr_distrib *d, int n);                                       /* setFFTSize :15-18; read at the next push */
int  csdr_distrib_set_lines_per_second(csdr_distrib *d, int lps);                             /* setLinesPerSecond :20-22 */
/* one popped input (:41-143): n_samples complex samples at iq with inp->frequency and inp->sampleRate; *n_lines (may be NULL) = lines emitted */
int  csdr_distrib_push(csdr_distrib *d, const float *iq, int iq_is_dev, int n_samples, int64_t frequency, int64_t sample_rate, int *n_lines);
int  csdr_distrib_get_state(const csdr_distrib *d, csdr_distrib_state *st);
int  csdr_distrib_lines(csdr_distrib *d, const float **dev_lines, int *n_lines, int *line_len); /* the last push's batch where it lies in HBM */
/* the last push's lines / the carried samples to the host (2 floats per sample; synchronise the distributor's stream): tests, host consumers */
int  csdr_distrib_fetch_lines(csdr_distrib *d, float *host, int64_t cap_floats, int *n_lines);
int  csdr_distrib_fetch_buffered(csdr_distrib *d, float *host, int64_t cap_floats, int *n_samples);
/* The last push's lines through SpectrumVisualProcessor::process, one input each, in order (the queue between the two in FFTVisualDataThread.cpp:58-70).
 * Full-span view: ONE csdr_spec_process(dev_lines, 1, n_lines, line_len, mode) -- CSDR_SPEC_FIRST_FRAME for lines of at least
 * csdr_spec_desired_input_size samples (what FFTVisualDataThread asks the distributor for), CSDR_SPEC_LINES for shorter ones; so the spectrum needs
 * max_frames >= n_lines and csdr_spec_frames / csdr_spec_fetch / csdr_waterfall_step_spec see n_lines frames.  Zoomed view: one call per line
 * (every call is one input there).  A push that emitted no line leaves the spectrum untouched.  Both handles are used by this call. */
int  csdr_spec_process_distrib(csdr_spec *spec, csdr_distrib *d);

/* ------------------------------------------------------------------ Spectrum bank: one SpectrumVisualProcessor per demodulator
 * The reference shows a spectrum and a waterfall of the ACTIVE demodulator (CubicSDR.cpp:373-381, DEFAULT_DMOD_FFT_SIZE 1024): one
 * SpectrumVisualProcessor fed the demodulator's resampled IQ.  A csdr_specbank holds max_slots of them, all of one fft_size F (internal size
 * Fi = 2 F: SPECTRUM_VZM, SpectrumVisualProcessor.h:11); the state of every slot and the points of every frame stay in HBM, and one call runs all
 * slots and all inputs it is given in ONE kernel launch.  Every slot behaves as one SpectrumVisualProcessor after setup(F), in full-span view
 * (is_view false, visualRatio 1), that receives one process() input per item.  Lines are those of src/process/SpectrumVisualProcessor.cpp.
 * 1. Limits.  F is a power of two, 8 <= F <= 2048 (Fi <= 4096 is what the transform holds in LDS); 1 <= max_slots <= 4096; max_frames >= 1 is the
 *    number of output frames a slot can hold per call.  F < 8, max_slots or max_frames out of range: CSDR_EINVAL; an F from 8 on that is not a power
 *    of two or exceeds 2048 -- sizes the reference takes (setFFTSize :180-190) -- CSDR_EUNSUPPORTED.  A call that would give a slot more frames than
 *    max_frames is refused as a whole with CSDR_ERANGE: nothing is processed and no state changes.
 * 2. Frame selection (:387-421), planned on the host per (slot, item) from the lengths alone.  lastDataSize is per slot, 0 after setup or reset.
 *      n >= Fi: the first Fi samples are the frame and become fftLastData; lastDataSize is not touched (:401-404).
 *      n < Fi and lastDataSize + n < Fi: priming.  num_copy = max(Fi - lastDataSize, n); fftLastData[0 .. num_copy) takes the data followed by
 *        zeros, no frame is produced, lastDataSize += num_copy (:407-413).
 *      otherwise the frame is fftLastData[lastDataSize - (Fi - n) .. lastDataSize) followed by the n new samples, and becomes fftLastData (:415-419).
 *    The reference's quirk is kept: a slot whose first inputs were >= Fi long still primes on its first short input.
 *    The library's own definition: an item with n = 0 is no input at all -- it advances no countdown and touches no state.  A block the front-end
 *    skipped (csdr_block_result.skipped) is such an item.
 * 3. Per frame (:437-576, :626-627), literally: the forward FFT of Fi points; the float magnitude with the half swap (:441-452); the NaN re-seeding
 *    and the two double averagers in the reference's order (:494-498); ceiling and floor (:500-505; their `!=` halves cannot fire: a float that
 *    only takes values through `>` / `<` never turns NaN); the four trackers at 0.05 with their re-seeding (:513-521) from 100 / 100 / 0 / 0 (:32-33);
 *    the display points, two bins per point, bin 0 replaced by fft_floor_maa (:542-576), log10 in double; fft_ceiling = point_ceil / sf,
 *    fft_floor = point_floor.  The average rate (default 0.65f, held as float) and the scale factor (default 1) are per object and are read by the
 *    next process call.  Output per frame: F y values; the x of point i is (float)i / (float)F and is added by the fetch, which returns (x, y)
 *    pairs as csdr_spec_fetch does.
 * 4. Peak hold (:115-125, :247, :264-273, :506-510, :523-530, :539-540): a per-object setter, per-slot state.  csdr_specbank_set_peak_hold is
 *    setPeakHold on every slot: the countdown to the reset becomes 1, or PEAK_RESET_COUNT = 30 when hold was on and is enabled again.  The
 *    countdown is decremented per non-empty item of a slot, on the host; the reset of fft_result_peak / fft_ceil_peak / fft_floor_peak happens on
 *    the device in front of the item it belongs to.  Hold points are fetched with csdr_specbank_fetch_hold; *n_floats = 0 when the frame carries none.
 * 5. Slot life cycle.  csdr_specbank_reset_slot makes a slot a fresh processor on which setPeakHold(the object's setting) was called once:
 *    averagers zero, trackers at their initial values, lastDataSize 0, the countdown at 1.  csdr_specbank_setup resets all slots (the object's
 *    average rate, scale factor and peak-hold setting stay).  Slots are independent: what one slot is fed, and whether others are fed at all,
 *    changes no bit of another slot's output; items of one slot are its inputs in the order given, whatever lies between them.
 * 6. Not in this object, and refused or absent rather than approximated: the zoomed view (the reference's demodulator view zooms the CHANNEL row;
 *    this bank shows the demodulator's own band at its own rate), hideDC, sizes that are not powers of two, F > 2048.  The zoomed view per slot,
 *    with hideDC, is an object of its own: csdr_viewbank ("View bank" below).
 * Ordering.  All work runs on a stream of the object's own, as a waterfall's does; the fetches synchronise it.  Host inputs are staged with
 * hipMemcpyAsync (the rule of csdr_post_execute for page-locked memory holds); device inputs must have been produced on the boundary stream.
 * csdr_specbank_process_bank orders itself behind the bank's front-end by an event and leaves one that the bank's later executes wait for before
 * that parity's buffers are rewritten: the two objects never synchronise the host for each other (a call waits on the host only for the upload of its
 * plan that last used the same page-locked staging set, two calls ago).  A refused call enqueues nothing and changes nothing.
 * The points are rewritten by the next process call.  ONE reader is waited for: csdr_wfbank_step_specbank ("Waterfall bank" below) leaves an event
 * behind its reads, and the next process, process_bank, setup or reset_slot waits for it on the device.  Any other reader of the pointer
 * csdr_specbank_device_points hands out is still not waited for: it has FINISHED before that call (csdr_waterfall_fetch_* or any other synchronising
 * call on the reader's stream). */
typedef struct csdr_specbank_item {
    int32_t slot;              /* 0 .. max_slots - 1 */
    int32_t n;                 /* complex samples of this process() input; 0: no input */
    const float *iq;           /* interleaved (re, im); device memory (8-byte aligned) when is_dev != 0 */
    int32_t is_dev;
    int32_t reserved;
} csdr_specbank_item;
CSDR_STATIC_ASSERT(sizeof(csdr_specbank_item) == 24 && offsetof(csdr_specbank_item, iq) == 8 && offsetof(csdr_specbank_item, is_dev) == 16, "csdr_specbank_item layout");
int  csdr_specbank_create(csdr_ctx *ctx, csdr_specbank **out);
void csdr_specbank_destroy(csdr_specbank *sb);
int  csdr_specbank_setup(csdr_specbank *sb, int fft_size, int max_slots, int max_frames);
int  csdr_specbank_set_average_rate(csdr_specbank *sb, float rate);       /* setFFTAverageRate */
int  csdr_specbank_set_scale_factor(csdr_specbank *sb, float sf);         /* setScaleFactor */
int  csdr_specbank_set_peak_hold(csdr_specbank *sb, int enabled);         /* setPeakHold :115-125, on every slot */
int  csdr_specbank_get_peak_hold(const csdr_specbank *sb);
int  csdr_specbank_reset_slot(csdr_specbank *sb, int slot);
/* n_items process() inputs; the items of one slot are its inputs in the order given */
int  csdr_specbank_process(csdr_specbank *sb, const csdr_specbank_item *items, int n_items);
/* After a csdr_bank_execute (CSDR_ESTATE before the first): every configured, active slot s < max_slots of the bank gets one item per block of that
 * execute -- that block's resampled IQ where it lies in HBM (what csdr_bank_fetch_iq returns, cut by csdr_block_result.n_iq).  Analog, host-only
 * (CSDR_MODEM_HOST) and digital slots alike: they all have resampled IQ.  Both handles are used by this call. */
int  csdr_specbank_process_bank(csdr_specbank *sb, csdr_bank *bank);
int  csdr_specbank_frames(const csdr_specbank *sb, int slot);             /* frames the last process call produced for the slot */
/* SpectrumVisualData of frame `frame` of the slot: spectrum_points[2 F] = (x, y) pairs, fft_ceiling, fft_floor (either may be NULL) */
int  csdr_specbank_fetch(csdr_specbank *sb, int slot, int frame, float *points_host, int cap_floats, double *fft_ceiling, double *fft_floor);
int  csdr_specbank_fetch_hold(csdr_specbank *sb, int slot, int frame, float *hold_host, int cap_floats, int *n_floats);
/* the y values of the slot's frames of the last call, [frames][F] floats in HBM: the boundary stream is made to wait for them, and they stay valid
 * until the next process or setup.  The pointer csdr_waterfall_step(points, is_dev = 1, n_floats_per_line = F, n_lines = frames) takes. */
int  csdr_specbank_device_points(csdr_specbank *sb, int slot, const float **dev, int *frames);

/* ------------------------------------------------------------------ Waterfall bank: one WaterfallPanel per demodulator
 * The reference draws the demodulator waterfall (DEFAULT_DMOD_FFT_SIZE 1024 x DEFAULT_DEMOD_WATERFALL_LINES_NB lines) of the ACTIVE demodulator:
 * one WaterfallPanel (src/panel/WaterfallPanel.cpp) fed by WaterfallCanvas::processInputQueue (src/visual/WaterfallCanvas.cpp:89-126).  A csdr_wfbank
 * holds max_slots of them, all of one fft_size and one `lines`; every slot's pending lines, kept points, two ring textures and picture stay in HBM,
 * and a step, an update or a render runs ALL the slots it concerns in ONE kernel launch.  Every slot behaves exactly as one csdr_waterfall does:
 * items 1 - 7 of "WaterfallPanel" and items 1 - 5 of "Waterfall viewport" above hold per slot, the reference's quirks (row lines - 1 unwritten during
 * the first turn, the older remainder above the newer run when an update crosses the wrap) and the library's own definitions (NaN -> index 0, the
 * texel rounding, which half a pixel shows, the LINEAR blend, the PEAK footprints) included.  What is per object and what per slot:
 * 1. Limits (setup :13-24 on every slot).  2 <= fft_size <= 4096, any value, half = fft_size / 2 <= 2048 (an odd last point is not drawn);
 *    2 <= lines <= 4096; 1 <= max_slots <= 4096; max_pending >= 1 lines may wait per slot; anything else is CSDR_EINVAL.  Per slot a setup clears
 *    lines_buffered, marks the textures uninitialised and keeps the points (:18-20: resized, new ones zero; a slot the object did not have before
 *    starts with zero points).  csdr_wfbank_reset_slot leaves ONE slot as after a setup, with its points zero; its neighbours are untouched.
 * 2. Gradient (item 5 above): one table for the object, the grey ramp before any csdr_wfbank_set_gradient; it outlives a setup.
 * 3. step.  An item is n_lines lines of n_floats_per_line floats for one slot: setPoints + step (:39-83) for each, with both line layouts, the
 *    wrong-length or NULL line that repeats the slot's previous points, and the steps dropped before the slot's first update -- their points are
 *    still kept -- as items 2 and 3 above state them, per slot.  The items of a slot are stepped in the order given, whatever lies between them;
 *    a wrong-length line directly behind a good one of the same call repeats that good line.  taken[i] (taken may be NULL) = the lines item i put
 *    into its slot's pending buffer.  A call that would leave ANY slot with more than max_pending lines waiting (CSDR_ERANGE), or that names a slot
 *    out of range (CSDR_EINVAL), is refused as a whole: it enqueues nothing and changes nothing, in no slot.
 * 4. step_specbank.  For every slot s below the smaller of the two objects' slot counts: the csdr_specbank_frames(sb, s) frames of the spectrum
 *    bank's last process, in frame order, straight from its point buffer in HBM -- one item per slot.  A spectrum bank whose fftSize is not fft_size
 *    delivers frames of the wrong size (item 2 above), as csdr_waterfall_step_spec defines for a spectrum.  *taken_total (may be NULL) = the lines
 *    taken over all slots.  What csdr_specbank_fetch returns is not changed by it.
 * 5. update is WaterfallPanel::update (:85-159) on every slot, and the panels are independent: a slot with at least one step call since its setup
 *    and no textures gets both rings zero-filled with waterfall_ofs = lines - 1; a slot with pending lines has them written by the reference's loop
 *    (item 4 above); a slot that was never stepped stays without textures.  So the slots' offsets differ as soon as their histories do.
 * 6. render is drawPanelContents (:161-219) of every listed slot scaled to width x height (limits and modes: viewport item 1; fft_size >= 4),
 *    as ONE dense RGBA8 picture of ceil(n_slots / atlas_cols) * height rows by atlas_cols * width pixels: the tile of list entry k lies at tile row
 *    k / atlas_cols, tile column k % atlas_cols, so atlas_cols = 1 gives [n_slots][height][width].  slots == NULL means slots 0 .. n_slots - 1
 *    (n_slots <= max_slots then); a slot may appear more than once; 1 <= atlas_cols <= n_slots <= 2^20.  A tile is byte for byte what
 *    csdr_waterfall_render_view(width, height, mode) gives for a waterfall in that slot's state; with width = 2 half, height = lines and PEAK it
 *    equals csdr_waterfall_fetch_rgba(0, lines), so there is no separate unscaled call.  THE LIBRARY'S OWN DEFINITION: the tile of a slot without
 *    textures (the reference draws nothing, :162-164) and the unused tiles of the last tile row are all-zero bytes -- transparent black --
 *    rewritten on every call.  out_u8 == NULL leaves the picture on the device; otherwise it is copied and the stream synchronised; too small a cap
 *    is CSDR_ERANGE.  A refusal renders nothing and changes nothing.  csdr_wfbank_device_view returns the last rendered picture and its size in
 *    pixels and makes the context's boundary stream wait for it; it stays valid until the next render or setup.
 * Ordering.  All work runs on a stream of the object's own; csdr_wfbank_fetch_index and a render into host memory synchronise it.  Host lines are
 * copied into page-locked staging inside the call, so the caller's buffer is free when it returns; device lines must have been produced on the
 * boundary stream, are ordered behind it by an event and stay unchanged until the next synchronising call on this object.  step_specbank makes the
 * object's stream wait for the spectrum bank's kernel by an event and leaves one that the spectrum bank's next process, process_bank, setup or
 * reset_slot waits for before it rewrites the points: the two objects never synchronise the host for each other.  A call waits on the host only for
 * the upload of its records that last used the same page-locked staging set, two calls ago. */
typedef struct csdr_wfbank_item {
    int32_t slot;              /* 0 .. max_slots - 1 */
    int32_t n_floats_per_line; /* fft_size, or 2 * fft_size for (x, y) pairs; anything else repeats the slot's previous points */
    const float *points;       /* n_lines lines, dense; device memory (4-byte aligned) when is_dev != 0; NULL repeats the previous points */
    int32_t is_dev;
    int32_t n_lines;           /* 0: nothing, not even a step call */
} csdr_wfbank_item;
CSDR_STATIC_ASSERT(sizeof(csdr_wfbank_item) == 24 && offsetof(csdr_wfbank_item, points) == 8 && offsetof(csdr_wfbank_item, is_dev) == 16 &&
                   offsetof(csdr_wfbank_item, n_lines) == 20, "csdr_wfbank_item layout");
int  csdr_wfbank_create(csdr_ctx *ctx, csdr_wfbank **out);
void csdr_wfbank_destroy(csdr_wfbank *wb);
int  csdr_wfbank_setup(csdr_wfbank *wb, int fft_size, int lines, int max_slots, int max_pending);
int  csdr_wfbank_set_gradient(csdr_wfbank *wb, const float *rgb_stops, int n_colors);        /* csdr_design_gradient's stops, as csdr_waterfall_set_gradient */
int  csdr_wfbank_reset_slot(csdr_wfbank *wb, int slot);
int  csdr_wfbank_step(csdr_wfbank *wb, const csdr_wfbank_item *items, int n_items, int *taken);      /* taken[n_items], may be NULL */
int  csdr_wfbank_step_specbank(csdr_wfbank *wb, csdr_specbank *sb, int *taken_total);        /* both handles are used by this call */
int  csdr_wfbank_update(csdr_wfbank *wb);                                                    /* WaterfallPanel::update on every slot */
int  csdr_wfbank_lines_buffered(const csdr_wfbank *wb, int slot);
int  csdr_wfbank_offset(const csdr_wfbank *wb, int slot, int half);                          /* waterfall_ofs[half] of the slot; -1 while it has no textures */
/* one ring texture of one slot: lines x (fft_size / 2) bytes, rows as GL holds them (synchronises); CSDR_ESTATE while the slot has no textures */
int  csdr_wfbank_fetch_index(csdr_wfbank *wb, int slot, int half, uint8_t *out_u8, int64_t cap);
int  csdr_wfbank_render(csdr_wfbank *wb, const int *slots, int n_slots, int width, int height, int mode, int atlas_cols, uint8_t *out_u8, int64_t cap);
int  csdr_wfbank_device_view(csdr_wfbank *wb, const uint8_t **dev, int *pic_width, int *pic_height);

/* ------------------------------------------------------------------ Scope bank: one ScopeVisualProcessor per demodulator
 * The reference feeds the audio scope of the ACTIVE demodulator from the demodulator's audio tap (DemodulatorThread.cpp:240-316): one
 * ScopeVisualProcessor (src/process/ScopeVisualProcessor.cpp:24-217; "ScopeVisualProcessor" above is the single object).  A csdr_scopebank holds
 * max_slots of them, all of one fft_size L; the state of every slot and the items of every frame stay in HBM, and one call runs all slots and all
 * frames it is given in TWO kernel launches (waveform, spectrum), whatever the slot count.  Every slot behaves exactly as one csdr_scope after
 * csdr_scope_setup(L, ...) that receives the slot's frames in the order given, whatever lies between them: its items are that object's byte for byte.
 * Lines are those of src/process/ScopeVisualProcessor.cpp.
 * 1. Limits (setup :24-35 on every slot).  L takes the values csdr_scope_setup takes: a power of two, 4 <= L <= 4096, otherwise CSDR_EUNSUPPORTED;
 *    1 <= max_slots <= 4096; max_frames >= 1 frames per slot and call; max_samples >= 1 floats per frame; otherwise CSDR_EINVAL.  Setup resets every
 *    slot; the object's settings (item 4) survive it.
 * 2. Frames.  An item is one AudioThreadInput for one slot, described by a csdr_scope_frame exactly as csdr_scope_process defines it: both layouts
 *    of a stereo tap read in place, n_dev (device frames only), scale, the three `type`s, one or two channels.  data_is_dev says where the data of
 *    ALL frames of the call lies.  THE LIBRARY'S OWN DEFINITION: an item with frame.n == 0 or frame.data == NULL is no input at all -- it touches no
 *    state and produces no item (the reference discards such inputs before process() does anything, :53-61).
 * 3. Per frame, literally what csdr_scope does (one statement of it serves both objects): the waveform item (:64-117) -- the peak search over
 *    min(n, maxScopeSamples) samples starting from 1.0f, every sample divided by it, x positions of the modes Y / 2Y / XY -- and the spectrum item
 *    (:119-214) -- the L zero-padded reals (stereo: left + right), fft_execute, the double magnitude, the two double averagers (the second sees the
 *    UPDATED first, :176-177), double extrema, the four trackers at 0.05 from zero (:11-12, :186-190), log10 in double, and
 *    outSize = floor(L/2 * sampleRate / inputRate) points in float arithmetic (:194-200).
 * 4. Settings are per object, apply to every slot and are read by the next process call: csdr_scopebank_set_enabled (setScopeEnabled /
 *    setSpectrumEnabled :37-43; a half that is off produces no item, and a spectrum that is off advances no averager), csdr_scopebank_set_max_scope_samples
 *    (default DEFAULT_DMOD_FFT_SIZE = 1024, :13), csdr_scopebank_set_average_rate (default 0.65f, :10).
 * 5. Slot life cycle.  csdr_scopebank_reset_slot makes a slot a fresh processor: both averagers and the four trackers zero; its neighbours are
 *    untouched.  Slots are independent: what one slot is fed, and whether others are fed at all, changes no bit of another slot's items.
 * 6. Refusals are whole-call -- they enqueue nothing and change nothing, in no slot: a slot out of range, channels not 1 or 2, a layout not 0 .. 2,
 *    n < 0: CSDR_EINVAL; a frame of more than max_samples floats: CSDR_ERANGE; more than max_frames frames for one slot: CSDR_ERANGE.
 * 7. process_bank.  After a csdr_bank_execute (CSDR_ESTATE before the first): every configured, active slot s below the smaller of the two objects'
 *    slot counts gets one item -- the frame csdr_bank_scope_frame(bank, s) describes, read where it lies in HBM.  A slot whose frame has n = 0 gets
 *    none: skipped blocks, front-end-only, host and digital slots.  A tap longer than max_samples refuses the call (item 6; the stereo tap is up to
 *    4096 floats).  Both handles are used by this call.
 * 8. Output.  csdr_scopebank_frames(slot) = the frames of the last process call for the slot; csdr_scopebank_fetch is csdr_scope_fetch per slot
 *    (which = 0 the waveform, 1 the spectrum; info->n_floats == 0 when that half was switched off).  csdr_scopebank_device_points hands out the
 *    slot's items of the last call where they lie in HBM: frame f at dev + f * stride_floats, stride_floats = L for the spectrum and
 *    2 * max_samples for the waveform; *frames = 0 when that half was switched off.  The boundary stream is made to wait for them.  A spectrum frame
 *    with sample_rate == input_rate holds L floats = L/2 (x, y) pairs: the pair layout csdr_wfbank_step / csdr_waterfall_step take for
 *    fft_size = L/2 (n_floats_per_line = L), so an audio waterfall per demodulator needs no raster code of its own.
 * 9. Not in this object: a raster of the waveform trace -- that is csdr_tracebank ("Trace bank" below), which reads the waveform items where
 *    csdr_scopebank_device_points hands them out; the tap of blocks other than the last one of an execute (the reference's one-deep queue
 *    shows at most one per display refresh); L above 4096.
 * Ordering.  All work runs on a stream of the object's own, as the spectrum bank's does; the fetches synchronise it.  Host frames are copied into
 * page-locked staging inside the call, so the caller's buffers are free when it returns; device frames must have been produced on the boundary stream
 * and are ordered behind it by an event.  csdr_scopebank_process_bank orders itself behind the bank's modem / audio kernels by an event and leaves one
 * that the bank's NEXT execute waits for on the device before it rewrites the taps (they are single-buffered): the two objects never synchronise the
 * host for each other.  A call waits on the host only for the upload of its plan that last used the same page-locked staging set, two calls ago.
 * The items are rewritten by the next process call.  A reader of the pointer csdr_scopebank_device_points hands out is NOT waited for: it has FINISHED
 * before the next process, process_bank, setup or reset_slot of this object (csdr_waterfall_fetch_* or any other synchronising call on the reader's
 * stream). */
typedef struct csdr_scopebank_item {
    int32_t slot;              /* 0 .. max_slots - 1 */
    int32_t reserved;
    csdr_scope_frame frame;    /* one AudioThreadInput; n == 0 or data == NULL: no input */
} csdr_scopebank_item;
CSDR_STATIC_ASSERT(sizeof(csdr_scopebank_item) == 56 && offsetof(csdr_scopebank_item, frame) == 8, "csdr_scopebank_item layout");
int  csdr_scopebank_create(csdr_ctx *ctx, csdr_scopebank **out);
void csdr_scopebank_destroy(csdr_scopebank *sb);
int  csdr_scopebank_setup(csdr_scopebank *sb, int fft_size, int max_slots, int max_frames, int max_samples);
int  csdr_scopebank_set_enabled(csdr_scopebank *sb, int scope_enabled, int spectrum_enabled);  /* :37-43, on every slot */
int  csdr_scopebank_set_max_scope_samples(csdr_scopebank *sb, int n);                          /* maxScopeSamples, default 1024 (:13) */
int  csdr_scopebank_set_average_rate(csdr_scopebank *sb, float rate);                          /* fft_average_rate, default 0.65 (:10) */
int  csdr_scopebank_reset_slot(csdr_scopebank *sb, int slot);
/* n_items AudioThreadInputs; the items of one slot are its frames in the order given */
int  csdr_scopebank_process(csdr_scopebank *sb, const csdr_scopebank_item *items, int n_items, int data_is_dev);
int  csdr_scopebank_process_bank(csdr_scopebank *sb, csdr_bank *bank);                         /* both handles are used by this call */
int  csdr_scopebank_frames(const csdr_scopebank *sb, int slot);                                /* frames of the last process call for the slot */
int  csdr_scopebank_fetch(csdr_scopebank *sb, int slot, int frame, int which, float *points_host, int cap_floats, csdr_scope_info *info);
int  csdr_scopebank_device_points(csdr_scopebank *sb, int slot, int which, const float **dev, int *frames, int *stride_floats);

/* ------------------------------------------------------------------ audio egress
 * csdr_mix replaces the arithmetic AND the queue rules of audioCallback (src/audio/AudioThread.cpp:88-240): sources in binding order;
 * a source takes part in a callback buffer only while bound, active and with a non-empty queue (:117); its first callback only latches a
 * block (:121-129); blocks at another sample rate are discarded (:131-149); mono samples feed both output channels (:169-194), stereo
 * ones are added float by float (:196-219); per source mixPeak = max(peak * gain) over the blocks it visited, and the buffer is scaled
 * by (float)(1 / sum) when the sum exceeds 1 (:222-238).  Samples live in per-source rings in HBM; every operation is individually
 * rounded in the callback's order, so the mix is the callback's bit for bit. */
int  csdr_mix_create(csdr_ctx *ctx, int max_sources, int ring_floats, int sample_rate, csdr_mix **out);
void csdr_mix_destroy(csdr_mix *mix);
int  csdr_mix_set_source(csdr_mix *mix, int source, int bound, int active, float gain, int queue_blocks);
/* one AudioThreadInput onto a source's queue (host or device memory); returns 1 when the queue was full and the block was dropped */
int  csdr_mix_push(csdr_mix *mix, int source, const float *audio, int is_dev, int n_floats, int channels, int sample_rate, float peak);
/* every block of the bank's last execute for n (slot, source) pairs: samples and peaks are appended in HBM by one kernel */
int  csdr_mix_push_bank(csdr_mix *mix, csdr_bank *bank, const int *slots, const int *sources, int n);
int  csdr_mix_queued(const csdr_mix *mix, int source);                  /* blocks waiting in the source's queue */
/* n_buffers consecutive callbacks of `frames` stereo frames -> out_host[n_buffers * frames * 2] (NULL: keep the result on the device) */
int  csdr_mix_render(csdr_mix *mix, int frames, int n_buffers, float *out_host);
/* AudioFileWAV::writePayloadToFileStream's conversion (src/audio/AudioFileWAV.cpp:133-157): int(x * (peak < 1 ? 32767 : 32767 / peak)),
 * low 16 bits.  Of the last render (peak: one value, or each buffer's summed peak), or of a demodulator's audio of the last execute --
 * every block with its own peak, as one AudioThreadInput each. */
int  csdr_mix_fetch_pcm16(csdr_mix *mix, int16_t *out_host, int cap_samples, float peak, int per_buffer_peak, int *n);
int  csdr_bank_fetch_pcm16(csdr_bank *bank, int slot, int16_t *out_host, int cap_samples, int *n);

/* ------------------------------------------------------------------ Squelch bank: level gate, gated mix and recorder per demodulator
 * DemodulatorThread::run decides per block whether anyone hears or records a demodulator's audio (src/demod/DemodulatorThread.cpp:142-238,
 * :318-345): signalLevel, signalFloor, signalCeil, squelchBreak, and the settings squelchEnabled, squelchLevel, muted.  A csdr_squelch holds them
 * for max_slots demodulators; the state of every slot and the items of every block stay in HBM, and one call steps every slot through every block
 * of a batch in ONE launch (squelch_scan); two more (squelch_pack, squelch_pcm16) write the recorder's stream.  Lines are those of
 * src/demod/DemodulatorThread.cpp unless a file is named.
 * 1. Limits.  1 <= max_slots <= 4096 (the packing kernel is one workgroup: 16 slots per thread), max_blocks >= 1; otherwise CSDR_EINVAL.
 * 2. Settings (csdr_squelch_set_slot): squelchEnabled (:392-397 switches it on with the level; here the caller says so), squelchLevel in dB, muted
 *    (:339-345), and the recorder option of AudioSinkFileThread.cpp:19-44.  THEY TAKE EFFECT AT THE NEXT PROCESS CALL AND ARE CONSTANT WITHIN IT: they
 *    are host values that travel with each call's plan.  The reference reads its atomics once per block, so a change made while a batch is in
 *    flight lands at a block boundary inside it there and at the batch boundary here.  Defaults: off, 0 dB, not muted, CSDR_RECORD_SILENCE.
 * 3. Per block of a slot, in block order (:142-220), the statements of host/DemodLevel.h: have_level = n_audio > 0 (:145);
 *    currentSignalLevel = 20 log10(max(level_accum / level_count, 1e-20)) in double (:59-67); sampleTime = double(n_in) / double(sample_rate);
 *    float trackers, updates in double, stored as float (:167-196); a block without audio still steps signalLevel towards 0 dB, which is what a
 *    digital slot does on every block.  No special cases beyond the reference's own.
 * 4. State.  A slot starts as the constructor leaves it (:20-27): -100, -30, 30, false.  csdr_squelch_reset_slot restores that and leaves the
 *    settings; reconfiguring the demodulator's slot in the bank does not reset (the reference's thread outlives its modem).  csdr_squelch_get_state
 *    reads the state after the last process: the meters (synchronises).
 * 5. Items.  One per stepped block: level, floor, ceil after the step and flags -- bit 0 squelched (:198), bit 1 squelchBreak after the step
 *    (:200-220; the solo-mode lock is GUI state and stays out), bit 2 open = !squelched && !muted, the condition of the audio push (:318-328).
 * 6. csdr_squelch_process: explicit inputs, one csdr_squelch_input per slot, so that the object is usable without a csdr_bank.  `blocks` is host
 *    memory; `audio` (optional: the recorder needs it, the level step does not) holds the blocks' floats back to back in host memory (copied inside
 *    the call) or, with audio_is_dev, in device memory produced on the boundary stream, which must stay valid until the call's work is done.
 *    Slots not named keep their state and report 0 blocks.
 * 7. csdr_squelch_process_bank: the bank's last execute, read where it lies in HBM (the level sums, the peaks, the block plan, the audio).  A slot
 *    is stepped when it is configured and active, has results in that execute, was not skipped by the shift rule (an unpushed block never reaches
 *    DemodulatorThread) and is not front-end-only (CSDR_MODEM_HOST: its level is the plug-in's to form).  n_in = the block's n_iq, sample_rate = the
 *    slot's bandwidth.  Digital slots step with have_level false.  Every other slot keeps its state and reports 0 blocks.  Both handles are used by
 *    this call; slots at or above the smaller of the two slot counts are not looked at.
 * 8. Recorder.  A slot's batch goes through AudioFileWAV's conversion (src/audio/AudioFileWAV.cpp:133-157, the rule of csdr_bank_fetch_pcm16), each
 *    block with its own audio_peak.  CSDR_RECORD_SILENCE: squelched blocks as zeros of the same length; CSDR_RECORD_SKIP_SILENCE: squelched blocks
 *    left out; CSDR_RECORD_ALWAYS: as if there were no squelch (AudioSinkFileThread.cpp:27-44).  `muted` does not affect the recorder.
 *    csdr_squelch_record copies every stepped slot's PCM16, packed in slot order, and offsets[max_slots + 1] (slot s: samples offsets[s] ..
 *    offsets[s + 1]): one small copy and one packed copy whatever the slot count.  A slot without audio records nothing.
 * 9. csdr_mix_push_squelched is csdr_mix_push_bank for the open blocks only: one queue entry per open block, in order, with its own peak -- the
 *    entries the host would have made with csdr_mix_push block by block.  It requires that the squelch bank's last process was
 *    csdr_squelch_process_bank of THIS bank's last execute (anything else: CSDR_ESTATE).  The mixer's queues are host state, so the call reads the
 *    flags once for the whole bank -- csdr_squelch_fetch_flags' copy, cached until the next process.  The all-or-nothing undo on a ring overrun
 *    and the stop at the first full queue are csdr_mix_push_bank's.
 * 10. Refusals are whole-call and change nothing: not created / no execute yet CSDR_ESTATE; a bank of another context CSDR_EINVAL; n_blocks above
 *    max_blocks (or negative), a slot out of range, the same slot twice in one process, a negative n_audio or n_in, a record option outside 0 .. 2:
 *    CSDR_EINVAL; an output capacity too small: CSDR_ERANGE.
 * Ordering.  All work runs on a stream of the object's own; only the calls that return data to the host synchronise it.  process_bank orders itself
 * behind the bank's modem / audio kernels by an event and leaves events that the bank's later executes wait for ON THE DEVICE before they rewrite
 * what was read (the audio and the sums: the next execute; the block plan: the second one after).  An execute issued straight behind process_bank
 * and csdr_squelch_record is therefore safe.  The pointer of csdr_squelch_device_items is for a consumer on the boundary stream, which is made to
 * wait for the items; such a reader has finished before the next process of this object. */
#define CSDR_RECORD_SILENCE      0
#define CSDR_RECORD_SKIP_SILENCE 1
#define CSDR_RECORD_ALWAYS       2
#define CSDR_SQUELCH_SQUELCHED 1u   /* flag bit 0 */
#define CSDR_SQUELCH_BREAK     2u   /* flag bit 1 */
#define CSDR_SQUELCH_OPEN      4u   /* flag bit 2 */
typedef struct csdr_squelch_block {
    double  level_accum;       /* the block's magnitude sum and its term count (csdr_block_result) */
    int32_t level_count;
    int32_t n_in;              /* input samples of the block: sampleTime = n_in / sample_rate */
    int32_t n_audio;           /* floats of audio the block produced; 0: no level */
    float   audio_peak;
} csdr_squelch_block;
typedef struct csdr_squelch_input {
    int32_t slot;
    int32_t n_blocks;
    int32_t sample_rate;
    int32_t audio_is_dev;
    const csdr_squelch_block *blocks;   /* host, [n_blocks] */
    const float *audio;                 /* NULL, or sum(n_audio) floats */
} csdr_squelch_input;
typedef struct csdr_squelch_item { float level, floor, ceil; uint32_t flags; } csdr_squelch_item;
CSDR_STATIC_ASSERT(sizeof(csdr_squelch_block) == 24 && sizeof(csdr_squelch_input) == 32 && sizeof(csdr_squelch_item) == 16, "squelch bank layouts");
int  csdr_squelch_create(csdr_ctx *ctx, int max_slots, int max_blocks, csdr_squelch **out);
void csdr_squelch_destroy(csdr_squelch *sq);
int  csdr_squelch_set_slot(csdr_squelch *sq, int slot, int enabled, float level_db, int muted, int record_option);
int  csdr_squelch_reset_slot(csdr_squelch *sq, int slot);                                      /* ctor :20-27 */
int  csdr_squelch_get_state(csdr_squelch *sq, int slot, float *level, float *floor, float *ceil, int *squelch_break);
int  csdr_squelch_process(csdr_squelch *sq, const csdr_squelch_input *in, int n);
int  csdr_squelch_process_bank(csdr_squelch *sq, csdr_bank *bank);                             /* both handles are used by this call */
int  csdr_squelch_blocks(const csdr_squelch *sq, int slot);                                    /* blocks stepped by the last process */
int  csdr_squelch_fetch(csdr_squelch *sq, int slot, csdr_squelch_item *out, int cap, int *n);
int  csdr_squelch_fetch_flags(csdr_squelch *sq, uint8_t *out, int64_t cap_bytes);              /* [max_slots][max_blocks], 0 where nothing was stepped */
int  csdr_squelch_device_items(csdr_squelch *sq, const csdr_squelch_item **dev, int *stride_items);   /* slot s, block b: dev[s * stride_items + b] */
int  csdr_squelch_record(csdr_squelch *sq, int16_t *out_host, int64_t cap_samples, int64_t *offsets /* [max_slots + 1] */);
int  csdr_mix_push_squelched(csdr_mix *mix, csdr_bank *bank, csdr_squelch *sq, const int *slots, const int *sources, int n);

/* ------------------------------------------------------------------ View bank: the zoomed demodulator spectrum, one per demodulator
 * The reference's demodulator spectrum and waterfall are a zoomed view of the CHANNEL row: SDRPostThread pushes the active demodulator's channel
 * row, at the channel's centre and rate, into IQActiveDemodVisualDataOutput (SDRPostThread.cpp:289-291, :334, :386) and AppFrame keeps
 * getDemodSpectrumProcessor() in setView(true, centre, bandwidth) (AppFrame.cpp:785-792, :2317-2320).  A csdr_viewbank holds max_slots such
 * processors, all of one fft_size F (Fi = 2 F); state and points stay in HBM, and one call runs all slots and all inputs it is given in ONE kernel
 * launch.  Every slot behaves as one SpectrumVisualProcessor after setup(F) on which setView(true, centre, bandwidth) was called before its first
 * input, and which receives one process() input per item.  Lines are those of src/process/SpectrumVisualProcessor.cpp.
 * 1. Limits.  F is a power of two, 8 <= F <= 2048; 1 <= max_slots <= 4096; max_frames >= 1 frames per slot and call; max_samples >= 1 is the longest
 *    input.  Bad counts: CSDR_EINVAL; an F from 8 on that is not a power of two or exceeds 2048: CSDR_EUNSUPPORTED.  A view that needs more than 10
 *    half-band stages (resampleBw below rate / 1024), or one wider than 32 input rates (more than 64 bins per display point): CSDR_EUNSUPPORTED for
 *    that call.  An input longer than max_samples, or more than max_frames frames for a slot: CSDR_ERANGE for the whole call.  A negative sample
 *    rate: CSDR_EINVAL.  A refusal enqueues nothing and changes no state, neither on the host nor on the device.
 * 2. Per item {slot, n, iq, is_dev, frequency, sample_rate}, planned on the host from these integers alone -- no decision depends on a sample value.
 *    The head of process(): doPeak is taken before the countdown moves, the peak reset is enqueued in front of the item (:247, :264-273).
 *    sample_rate == 0 ends the input there (:284-287).  resampleBw comes from repeated long division by 2 while resampleBw / 2 >= bandwidth
 *    (:289-291; 503606 becomes 251803, then 125901: the truncation is kept); resamplerRatio is the double quotient (:293);
 *    desiredInputSize = (size_t)(Fi / ratio), clamped to n (:295-302): only that prefix of the input is consumed -- the oscillator advances by it and
 *    the resampler sees the concatenation of these prefixes.  Retune (:304-336), when centerFreq != frequency and the shift or the input rate changed:
 *    in range -- |frequency - centre| < sample_rate / 2, the application rate being the input's, as csdr_spec defines it -- shiftFrequency is adopted,
 *    the oscillator's increment becomes the phase word of (float)(2 pi |shift| / rate), and fft_result_ma / _maa move by
 *    numShift = floor(|freqDiff| / (lastBandwidth / Fi)) bins, left for a positive freqDiff, when 0 < numShift < Fi / 2 (the peak arrays do not
 *    move); peakReset = 30 is set whether or not the range test passed; out of range the old shift and increment keep mixing.  Mixing is up for
 *    shiftFrequency < 0, else down (:345-349); none, and no advance of the oscillator, when centerFreq == frequency (:351).  The resampler is
 *    rebuilt when there is none or resampleBw or the input rate changed (:354-368): msresamp_crcf_create((float)ratio, 60), every window empty,
 *    phase and buffer index 0, the oscillator's phase lives on; bwDiff, lastBandwidth, lastInputBandwidth and peakReset = 30 are set.
 *    num_written is that resampler's output count for the consumed samples, in closed form.  Then the frame rule of :399-421 on num_written,
 *    exactly as "Spectrum bank" item 2 states it, late-priming quirk included (an input whose num_written is 0 primes, or slides by nothing, as
 *    the rule says).  The stretch / squeeze of the averagers (:454-492) runs in front of the averaging of a frame when the resampler is new and the
 *    slot's previous input was a view input: squeeze (src = Fi/4 + i/2) for bwDiff < 0, else stretch (inside [Fi/4, Fi - Fi/4) take (i - Fi/4) 2,
 *    elsewhere 0).  last_view becomes true after every non-empty item, the early returns included.
 * 3. Per frame: the statements of "Spectrum bank" item 3, with two differences.  The display walks the view map of :532-560: the double accumulator
 *    is stepped by 2 bandwidth / resampleBw per point, idx = round(visualStart + i) as unsigned; a visited bin with 0 < idx < Fi contributes
 *    fft_result_maa[idx], any other fft_floor_maa; the sum is divided by the count and log10 is taken in double.  The host computes the map per slot
 *    and uploads it only when (bandwidth, resampleBw) changed.  The hold points walk the same map over fft_result_peak.  hideDC (:578-623, the
 *    reference's integer arithmetic) is a per-object setter and is applied BY THE KERNEL to points and hold points: what lies in HBM is what the
 *    reference hands its canvases.
 * 4. The library's own definitions.  An item with n = 0 is no input at all.  csdr_viewbank_set_view with bandwidth <= 0 is CSDR_EINVAL; a slot that
 *    was never given a view is refused with CSDR_ESTATE when fed.  csdr_viewbank_reset_slot makes a fresh processor on which setPeakHold(the
 *    object's setting) and the slot's last setView were called; csdr_viewbank_setup makes every slot a processor without a view.  Slots share
 *    nothing: what one slot is fed changes no bit of another's output; however a slot's inputs are cut into calls, its output is the same bits.
 * Ordering.  All work runs on a stream of the object's own; the fetches synchronise it.  Host inputs are staged with hipMemcpyAsync; device inputs
 * must have been produced on the boundary stream.  csdr_viewbank_process_post waits on its stream for the channelizer batch's event and leaves one
 * of the batch's reader events behind its kernel: neither object synchronises the host for the other, and the post rotates its output buffers from
 * then on.  The points are rewritten by the next process call; a reader of csdr_viewbank_device_points' pointer must have FINISHED before it. */
typedef struct csdr_viewbank_item {
    int32_t slot;              /* 0 .. max_slots - 1 */
    int32_t n;                 /* complex samples of this process() input; 0: no input */
    const float *iq;           /* interleaved (re, im); device memory (8-byte aligned) when is_dev != 0 */
    int32_t is_dev;
    int32_t reserved;
    int64_t frequency;         /* the input's centre frequency (SpectrumVisualData::frequency) */
    int64_t sample_rate;       /* the input's sample rate (::sampleRate) */
} csdr_viewbank_item;
CSDR_STATIC_ASSERT(sizeof(csdr_viewbank_item) == 40 && offsetof(csdr_viewbank_item, iq) == 8 && offsetof(csdr_viewbank_item, frequency) == 24, "csdr_viewbank_item layout");
typedef struct csdr_viewbank_slot_state {      /* a slot's integers behind its last item */
    int64_t resample_bw;       /* resampleBw */
    int64_t shift_frequency;   /* shiftFrequency */
    int32_t desired_input_size;/* desiredInputSize (before the clamp to n) */
    int32_t last_data_size;    /* lastDataSize */
    int32_t peak_reset;        /* peakReset */
    int32_t num_written;       /* num_written of the last item */
} csdr_viewbank_slot_state;
CSDR_STATIC_ASSERT(sizeof(csdr_viewbank_slot_state) == 32, "csdr_viewbank_slot_state layout");
int  csdr_viewbank_create(csdr_ctx *ctx, csdr_viewbank **out);
void csdr_viewbank_destroy(csdr_viewbank *vb);
int  csdr_viewbank_setup(csdr_viewbank *vb, int fft_size, int max_slots, int max_frames, int max_samples);
int  csdr_viewbank_set_average_rate(csdr_viewbank *vb, float rate);       /* setFFTAverageRate */
int  csdr_viewbank_set_scale_factor(csdr_viewbank *vb, float sf);         /* setScaleFactor */
int  csdr_viewbank_set_peak_hold(csdr_viewbank *vb, int enabled);         /* setPeakHold :115-125, on every slot */
int  csdr_viewbank_get_peak_hold(const csdr_viewbank *vb);
int  csdr_viewbank_set_hide_dc(csdr_viewbank *vb, int enabled);           /* setHideDC :204-209, on every slot */
int  csdr_viewbank_set_view(csdr_viewbank *vb, int slot, int64_t center_freq, int64_t bandwidth);     /* setView(true, ...) :64-72 */
int  csdr_viewbank_reset_slot(csdr_viewbank *vb, int slot);
/* n_items process() inputs; the items of one slot are its inputs in the order given */
int  csdr_viewbank_process(csdr_viewbank *vb, const csdr_viewbank_item *items, int n_items);
/* After a csdr_post_execute (CSDR_ESTATE before the first): slot slots[i] gets one item per block of that execute -- that block of row channels[i]
 * where it lies in the post's buffer, stamped with the centre and csdr_post_channel_rate that csdr_bank_execute uses for that row.  CSDR_ERANGE when
 * the batch already has its four readers; CSDR_EINVAL for a post of another context, a packed-row producer, a row the channelizer does not
 * produce.  No host synchronisation in either direction.  Both handles are used by this call. */
int  csdr_viewbank_process_post(csdr_viewbank *vb, csdr_post *post, const int *slots, const int *channels, int n);
int  csdr_viewbank_frames(const csdr_viewbank *vb, int slot);             /* frames the last process call produced for the slot */
/* SpectrumVisualData of frame `frame` of the slot: spectrum_points[2 F] = (x, y) pairs, fft_ceiling, fft_floor (either may be NULL) */
int  csdr_viewbank_fetch(csdr_viewbank *vb, int slot, int frame, float *points_host, int cap_floats, double *fft_ceiling, double *fft_floor);
int  csdr_viewbank_fetch_hold(csdr_viewbank *vb, int slot, int frame, float *hold_host, int cap_floats, int *n_floats);
/* the y values of the slot's frames of the last call, [frames][F] floats in HBM: the boundary stream is made to wait for them.  The pointer
 * csdr_wfbank_step / csdr_waterfall_step take with is_dev = 1. */
int  csdr_viewbank_device_points(csdr_viewbank *vb, int slot, const float **dev, int *frames);
int  csdr_viewbank_slot_info(const csdr_viewbank *vb, int slot, csdr_viewbank_slot_state *out);
/* the slot's fftLastData, 2 Fi floats (synchronises): the resampler's samples as the frame rule arranged them */
int  csdr_viewbank_fetch_last(csdr_viewbank *vb, int slot, float *out, int cap_floats);

/* ------------------------------------------------------------------ Trace bank: spectrum and scope lines as RGBA tiles
 * The lines the reference draws above and beside the waterfall: the spectrum trace with its peak-hold trace (src/panel/SpectrumPanel.cpp:117-160)
 * and the scope trace in its three modes (src/panel/ScopePanel.cpp:30-112).  A csdr_tracebank draws any number of polylines -- read where the
 * spectrum, view and scope banks left them in HBM, or given on the host -- into ONE dense RGBA8 atlas with the tile geometry of csdr_wfbank_render,
 * so the trace of list entry k lies over the waterfall tile of list entry k.  One launch draws every item of the line kinds, one every XY item,
 * whatever the item count, and no point of the input is lost.  THE PICTURE IS THE LIBRARY'S OWN DEFINITION: GL_LINE_SMOOTH is implementation-defined
 * and the reference has no pixel oracle, so, as with the waterfall's texel rounding, this block defines the picture and every implementation is held
 * to it byte for byte.  After one float step per vertex everything is exact integer arithmetic (64-bit wherever a product could pass 2^31).
 * 1. Quantiser.  A value y of a kind with constants (y0, s) -- (0, 1) for CSDR_TRACE_SPECTRUM, (-1, 0.5f) for the scope kinds -- in a panel of H rows:
 *    u = (y - y0) * s, each operation rounded to float on its own; q = (int)floorf(u * (float)H) clamped to [0, H - 1]; u < 0 and -0.0 give 0, u >= 1
 *    and +inf give H - 1, NaN gives 0.  The row is r = H - 1 - q, row 0 at the top.  The XY kind quantises x the same way into a column, with the tile
 *    width in place of H and without the flip.
 * 2. Columns.  A polyline has n >= 1 vertices; vertex i lies in column c_i = floor(i * W / n) of a tile W pixels wide -- the reference's
 *    x = (float)i / (float)F (SpectrumVisualProcessor.cpp:542-576) and ((double)i / iMax - 0.5) * 2 (ScopeVisualProcessor.cpp:111).  The x of an
 *    (x, y) pair is not read by the line kinds.  The trace ends in column c_{n-1}: short of the right edge when n < W, as the reference's.
 * 3. Segments.  For vertices i, i + 1 with a = c_i, b = c_{i+1}, ra = r_i, rb = r_{i+1}: if a == b, column a receives the rows ra and rb.  Otherwise,
 *    with d = b - a, every column c in [a, b] receives the two rows ra + rdiv((rb - ra) * t, 2 d) for t = clamp(2 (c - a) - 1, 0, 2 d) and
 *    t = clamp(2 (c - a) + 1, 0, 2 d), where rdiv(p, q) = floor((2 p + q) / (2 q)) -- a floor division for negative p too.  A column's lit interval
 *    [lo, hi] is the hull of everything it received (for n == 1 the single vertex); a column that received nothing is unlit.  So every column up to
 *    c_{n-1} is lit, every vertex's row lies in its column's interval, and the intervals of adjacent columns share a row: the trace is connected and
 *    loses no peak.  Rows [0, 9, 0] at W = 7 give lo = [0, 2, 7, 2, 0, -, -], hi = [2, 7, 9, 7, 2, -, -].
 * 4. Kinds.  `n` counts vertices for the line kinds: layout 0 is n y values, layout 1 is n (x, y) pairs (what the fetches return and what the scope
 *    bank's waveform items hold).
 *    CSDR_TRACE_SPECTRUM (SpectrumPanel.cpp:149-160): one polyline of n vertices; if `hold` is not NULL, a second one of n vertices in the same
 *      layout drawn over it: where the hold interval covers a pixel, out_c = (dst_c + hold_c + 1) >> 1 per colour channel (the reference's 0.5 alpha).
 *      The dB grid and the frequency labels stay out of this object: they are csdr_overlay's ("Overlay bank" below).
 *    CSDR_TRACE_SCOPE_Y (ScopePanel.cpp:32-44, :97-99): one polyline; under it the row of y = 0 in the minor axis colour.
 *    CSDR_TRACE_SCOPE_2Y (:45-67, :100-105, constructor :7-16; height >= 2): an upper sub-panel of H / 2 rows and a lower one of H - H / 2.  The
 *      first n / 2 vertices are drawn in the upper one, the next n / 2 in the lower one, each as a polyline of n / 2 vertices over the full width;
 *      an odd last vertex is not drawn, and n == 1 draws the axes alone.  Each sub-panel is a panel of its own height with its own y = 0 row in the
 *      minor colour; the first row of the lower sub-panel is in the major colour.
 *    CSDR_TRACE_SCOPE_XY (:69-82, :88-89, :106-108): here n counts FLOATS, n / 2 points (x, y), whatever the layout says; a pixel hit k times is
 *      min(255, bg_c + k * line_c) per channel (GL_ONE, GL_ONE).  The reference's 0.05-alpha background -- its persistence across frames -- stays out:
 *      every render starts from the background.
 * 5. Paint order per tile: background, minor axis rows, major axis row, line, hold.  Alpha is the background's alpha wherever a tile is drawn.
 *    Colours are caller data, one set per object: bg RGBA; line, hold, axis_major, axis_minor RGB bytes; before any csdr_tracebank_set_colors:
 *    black / 255, white, (0, 255, 0), white, (89, 89, 89).  A NULL argument of set_colors leaves that colour as it is.
 * 6. Atlas: exactly csdr_wfbank_render's (item 6 of "Waterfall bank").  ceil(n_items / atlas_cols) * height rows by atlas_cols * width pixels; entry k
 *    at tile row k / atlas_cols, tile column k % atlas_cols.  The tile of an item with n == 0 or points == NULL and the unused tiles of the last tile
 *    row are all-zero bytes, rewritten on every call.  out_u8 == NULL leaves the picture on the device; csdr_tracebank_device_view returns the last
 *    rendered picture and its size in pixels; it stays valid until the next render or setup.
 * 7. Limits.  2 <= width <= 16384, 1 <= height <= 16384, 1 <= atlas_cols <= n_items <= max_items <= 2^20, 0 <= n <= max_points, 1 <= max_points
 *    <= 2^21.  A kind or a layout out of range, bits of is_dev other than the two below, n < 0, 2Y at height 1, or device points that are not 4-byte
 *    aligned: CSDR_EINVAL.  n above max_points, or a host buffer too small: CSDR_ERANGE.  A refusal renders nothing and changes nothing.
 * 8. csdr_design_trace_envelope is items 1 - 4 on the host, no device needed: lo and hi hold 2 * width entries each -- [0, width) the line's intervals
 *    (2Y: the upper sub-panel's), [width, 2 width) the hold's (2Y: the lower sub-panel's; nothing otherwise), in tile rows, lo = hi = -1 for an unlit
 *    column.  CSDR_TRACE_SCOPE_XY has no envelope (CSDR_EINVAL); n == 0 leaves every column unlit; n above 2^21 is CSDR_ERANGE.
 * Ordering is the waterfall bank's.  All work runs on a stream of the object's own; a render into host memory synchronises it.  Host points are
 * copied into page-locked staging inside the call, so the caller's buffers are free when it returns.  Device points must have been produced on, or
 * handed to, the boundary stream -- what csdr_specbank_device_points, csdr_viewbank_device_points and csdr_scopebank_device_points do -- are ordered
 * behind it by an event and stay unchanged until the next synchronising call on this object.  csdr_tracebank_device_view makes the boundary stream
 * wait for the picture.  The producing banks are not touched and wait for nobody here: a caller who keeps the picture on the device (out_u8 == NULL)
 * synchronises this object -- a render into host memory, or csdr_tracebank_device_view and a synchronise of the boundary stream -- before the
 * producer's next process, the rule those device_points calls give every reader.  A call waits on the host only for the upload of its records that
 * last used the same page-locked staging set, two calls ago. */
#define CSDR_TRACE_SPECTRUM  0
#define CSDR_TRACE_SCOPE_Y   1
#define CSDR_TRACE_SCOPE_2Y  2
#define CSDR_TRACE_SCOPE_XY  3
#define CSDR_TRACE_DEV_POINTS 1  /* bits of csdr_trace_item.is_dev: `points` is device memory */
#define CSDR_TRACE_DEV_HOLD   2  /* `hold` is device memory */
typedef struct csdr_trace_item {
    const float *points;       /* the polyline (XY: the points); NULL: an empty tile */
    const float *hold;         /* CSDR_TRACE_SPECTRUM: the hold points, n vertices in the same layout, or NULL; not read by the other kinds */
    int32_t n;                 /* vertices (XY: floats); 0: an empty tile */
    int32_t layout;            /* 0: y values; 1: (x, y) pairs */
    int32_t kind;              /* CSDR_TRACE_* */
    int32_t is_dev;            /* CSDR_TRACE_DEV_* bits; device memory is 4-byte aligned */
} csdr_trace_item;
CSDR_STATIC_ASSERT(sizeof(csdr_trace_item) == 32 && offsetof(csdr_trace_item, hold) == 8 && offsetof(csdr_trace_item, n) == 16 &&
                   offsetof(csdr_trace_item, is_dev) == 28, "csdr_trace_item layout");
int  csdr_tracebank_create(csdr_ctx *ctx, csdr_tracebank **out);
void csdr_tracebank_destroy(csdr_tracebank *tb);
int  csdr_tracebank_setup(csdr_tracebank *tb, int max_items, int max_points);
int  csdr_tracebank_set_colors(csdr_tracebank *tb, const uint8_t *bg /*[4]*/, const uint8_t *line /*[3]*/, const uint8_t *hold /*[3]*/,
                               const uint8_t *axis_major /*[3]*/, const uint8_t *axis_minor /*[3]*/);
int  csdr_tracebank_render(csdr_tracebank *tb, const csdr_trace_item *items, int n_items, int width, int height, int atlas_cols, uint8_t *out_u8, int64_t cap);
int  csdr_tracebank_device_view(csdr_tracebank *tb, const uint8_t **dev, int *pic_width, int *pic_height);
int  csdr_design_trace_envelope(const float *points, const float *hold_or_null, int n, int layout, int kind, int width, int height,
                                int32_t *lo /*[2 width]*/, int32_t *hi /*[2 width]*/);

/* ------------------------------------------------------------------ Overlay bank: grid, frequency scale, markers and labels on the tiles
 * What tells a viewer what a tile shows: the dB grid (src/panel/SpectrumPanel.cpp:117-147), the frequency ticks with their MHz labels and the two dB
 * labels (:171-303), and a marker and a label for every demodulator (PrimaryGLContext::DrawDemodInfo, src/visual/PrimaryGLContext.cpp:65-199).  A
 * csdr_overlay composites ORDERED LISTS OF PRIMITIVES -- filled rectangles, optionally masked by a window of an 8-bit coverage plane (the glyphs of a
 * font) -- onto the tiles of an atlas in ONE launch whatever the tile count; the csdr_design_* planners below turn the reference's numbers into such
 * lists on the host, no device needed.  THE PICTURE IS THE LIBRARY'S OWN DEFINITION, all integer, and every implementation is held to it byte for byte.
 * 1. Atlas: exactly csdr_wfbank_render's (item 6 of "Waterfall bank"): ceil(n_tiles / atlas_cols) * height rows by atlas_cols * width pixels, RGBA8,
 *    tile k at tile row k / atlas_cols, tile column k % atlas_cols.  So tile k lies over tile k of csdr_tracebank_render / csdr_wfbank_render.
 * 2. Base.  `base` is a picture of that very size and is never modified: host memory; with base_is_dev != 0 device memory, 4-byte aligned -- what
 *    csdr_tracebank_device_view, csdr_wfbank_device_view or csdr_waterfall_device_view returned --; or NULL: all-zero bytes.  The output starts as the
 *    base's bytes.  The unused tiles of the last tile row are zero bytes whatever the base holds; a tile with count == 0 is the base's bytes.
 * 3. Lists.  tiles[k] = {first, count} names the run prims[first .. first + count) of the call's primitives as tile k's list; runs may overlap and
 *    may be shared between tiles.  A primitive covers the pixels x <= px < x + w, y <= py < y + h of its tile (row 0 at the top) that lie inside the
 *    tile: it may lie partly or wholly outside and is clipped; w == 0 or h == 0 draws nothing.
 * 4. The rule.  For each pixel of a tile the primitives of its list that cover it are applied IN LIST ORDER to its four bytes d = (R, G, B, A), with
 *    the primitive's colour bytes s = (rgba[0], rgba[1], rgba[2]) and its alpha a = rgba[3]:
 *      a_eff = a                             without a mask (mask_x < 0);
 *      a_eff = (a * cov + 127) / 255         with one, cov the font plane's byte at column mask_x + (px - x), row mask_y + (py - y): the window's
 *                                            origin belongs to the primitive's UNCLIPPED origin, so a glyph cut by a tile edge keeps its shape.
 *      CSDR_OVL_OVER  every byte: (s * a_eff + d * (255 - a_eff) + 127) / 255, with s = 255 for the A byte   (GL_SRC_ALPHA, GL_ONE_MINUS_SRC_ALPHA)
 *      CSDR_OVL_ADD   every byte: min(255, d + (s * a_eff + 127) / 255), with s = 255 for the A byte         (GL_SRC_ALPHA, GL_ONE)
 *      CSDR_OVL_COPY  R, G, B = s; A = a_eff
 *    All divisions are integer divisions of non-negative numbers.  a_eff == 0 leaves OVER and ADD pixels as they are; a_eff == 255 makes OVER a copy.
 * 5. Limits.  1 <= width, height <= 16384; 1 <= atlas_cols <= n_tiles <= max_tiles <= 2^20; 0 <= n_prims <= max_prims <= 2^22 (1 <= max_prims);
 *    w, h >= 0; |x|, |y| <= 2^20.  CSDR_EINVAL, whole-call: a size out of range; a run not inside [0, n_prims] (first < 0, count < 0 or
 *    first + count > n_prims); a mode out of range; w or h negative, |x| or |y| above 2^20; a masked primitive when no font is set, with mask_y < 0,
 *    or whose window [mask_x, mask_x + w) x [mask_y, mask_y + h) leaves the font plane; a device base that is not 4-byte aligned.  CSDR_ERANGE:
 *    n_tiles above max_tiles, n_prims above max_prims, a host buffer too small.  A refusal enqueues nothing and changes nothing: the last picture,
 *    csdr_overlay_device_view and the font stay as they were.
 * 6. Font.  csdr_overlay_set_font copies an 8-bit coverage plane of font_w x font_h bytes (1 .. 16384 each), dense, row 0 at the top, from host
 *    memory to the device (synchronises).  The plane is caller data: the product ships no font and decodes no image.  a8 == NULL removes the font.
 * 7. out_u8 == NULL leaves the picture on the device; csdr_overlay_device_view returns the last composed picture and its size in pixels and makes the
 *    boundary stream wait for it; it stays valid until the next compose or setup.
 * Ordering is the trace bank's.  All work runs on a stream of the object's own; a compose into host memory synchronises it.  The lists and a host base
 * are copied into page-locked staging inside the call (two sets, used in turn), so the caller's buffers are free when it returns; a device base must
 * have been produced on, or handed to, the boundary stream, is ordered behind it by an event and stays unchanged until the next synchronising call
 * on this object.
 *
 * Planners (host only, no device; they set no csdr_last_error).  NDC -> pixels is ONE rule for all of them, in double, in a view of W x H pixels:
 *      a horizontal boundary of u:            hb(u) = clamp(floor((u + 1) * 0.5 * W), 0, W)
 *      a vertical boundary of v, from the top: vb(v) = clamp(floor((1 - v) * 0.5 * H), 0, H)
 *    A rectangle between two boundaries is half-open -- columns [hb(u0), hb(u1)), rows [vb(v1), vb(v0)) for v0 < v1 -- so neighbours tile without gap
 *    or overlap.  A vertical line of k pixels at u is the k columns from hb(u) - k / 2 (integer division), a horizontal line of one pixel at v the row
 *    vb(v); both clipped to the view.  A float alpha or colour c becomes the byte (int)(c * 255 + 0.5).
 * a. csdr_design_freq_scale (SpectrumPanel.cpp:171-277).  With the reference's types -- long long leftFreq = (double)freq - (double)bandwidth / 2.0
 *    and rightFreq = leftFreq + (double)bandwidth, both truncated; LONG DOUBLE for mhzStep, mhzStart and currentMhz as the reference (the platform's
 *    long double: 80-bit on x86-64); double for m; float for viewWidth and viewHeight --:  mhzStep = (100000 / (rightFreq - leftFreq)) * 2, visual step
 *    0.1, precision 1.  While mhzStep * 0.5 * viewWidth < 40 * font_scale the ladder goes on to 0.25, 0.5, 1, 2.5, 5, 10 and 50 MHz (:184-216); else,
 *    if it exceeds 350 * font_scale, the step is 0.01 MHz and the precision 2 (:217-221).  firstMhz = (leftFreq / 1000000) * 1000000 with truncating
 *    division (:223), mhzStart = (firstMhz - leftFreq) / (rightFreq - leftFreq) * 2, currentMhz = trunc(floor(firstMhz / 1e6)).  The loop (:241-277)
 *    runs m from -1 + mhzStart in steps of mhzStep while m <= 1 + |mhzStart|; below -1 it skips (adding the visual step to currentMhz), above 1 it
 *    stops.  Per tick: m; value = currentMhz; label = "%.<precision>f" of it; major = (modf((double)currentMhz) < 0.001) (:255); column = hb(m).
 *    A tick whose m is exactly -1 or 1 may fall either way (the sum m += mhzStep is rounded).  Also: tick_top = lMhzPos = 1 - 5 / viewHeight,
 *    label_y = hPos = 1 - (16 / viewHeight) * font_scale and font_size 12, or 1 - (18 / viewHeight) * font_scale and 16 when viewHeight > 135, with
 *    their rows tick_rows = vb(tick_top) (a tick fills rows [0, tick_rows)) and label_row = vb(label_y).  A major tick is 4 pixels wide (:256), a
 *    minor one 1; the minor colour is 0.65 of the major one (:260).  bandwidth < 1, a view side outside 1 .. 16384, font_scale <= 0 or more than
 *    2^20 loop turns: CSDR_EINVAL; more ticks than cap: CSDR_ERANGE with out->n_ticks the number needed.
 * b. csdr_design_db_grid (:117-147).  range = ceil - floor in double from the two floats.  The three ranges {min, max, trans, step} = {90, 5000, 10,
 *    100}, {20, 150, 10, 10}, {-20, 30, 10, 1}, in that order; one applies when min <= range <= max, with alpha 1, times (range - min) / trans when
 *    range <= min + trans, times (trans - (range - (max - trans))) / trans when range >= max - trans.  Its positions: p starts at 0 and p += step / range
 *    once per l = floor, floor + step, ... while l <= ceil + step; EVERY p is returned, in order, on the panel or not (0 <= p <= 1 is on it: p is the
 *    height above the tile's bottom edge as a fraction of its height, the tile being the trace's panel, so its row is vb(2 p - 1)).  The colour is
 *    0.12 grey, blended CSDR_OVL_ADD.  THE GRID IS ADDED OVER A FINISHED TRACE TILE, not under the trace as in the reference: the two differ only
 *    where a trace pixel lies on a grid row.  floor or ceil not finite: CSDR_EINVAL; more positions than cap: CSDR_ERANGE.
 * c. csdr_design_db_labels (:281-303): both strings are "%.1fdB" of db_offset + 20 log10(2 v / fft_size), v the float ceil or floor; both are empty
 *    when ceil == floor or fft_size == 0.  (The gradient grounds of the two labels stay out.)
 * d. csdr_design_demod_marker (PrimaryGLContext.cpp:89-164, :168-197), in float as the reference: uxPos = ((float)(demod_freq - (center_freq -
 *    srate / 2)) / (float)srate - 0.5) * 2; ofs = (float)bandwidth / (float)srate; ofsLeft = 0 for CSDR_SIDEBAND_USB, ofsRight = 0 for
 *    CSDR_SIDEBAND_LSB, else ofs; labelHeight = 20 / viewHeight, hPos = -1 + labelHeight.  Up to four primitives, in the reference's order, between
 *    the columns hb(uxPos - ofsLeft) and hb(uxPos + ofsRight): the label ground, black at alpha 0.35, OVER, rows [vb(hPos + labelHeight), H) (:110-134);
 *    the band in `rgb` at alpha 0.2, ADD, over the full height (:136-145); the same once more over the ground's rows when ofs * 2 < 16 / viewWidth
 *    (:147-156: `narrow`); with CSDR_MARKER_CENTERLINE a one-pixel line at uxPos in `rgb` at alpha 0.5, ADD (:158-164).  The label: prefix "[" +
 *    ("V" if _DELTA_LOCK) + ("R" if _RECORDING) + ("M" if _MUTED, else "S" if _SOLO) + "] ", empty when no letter applies (:168-187); anchored at
 *    (label_x, label_y) = (hb(uxPos), vb(hPos)), vertically centred, horizontally left for USB, right for LSB, else centred (:191-197); white at
 *    alpha 0.8, OVER.  The solo and recording tints of the label ground (:112-124) are GUI state and a clock and stay out.  srate < 1 or a view side
 *    outside 1 .. 16384: CSDR_EINVAL.
 * e. csdr_design_text lays one string out as masked primitives, by the library's own rule.  A csdr_glyph table is caller data with BMFont's
 *    meaning: (x, y, w, h) the glyph's window in the plane, (xoffset, yoffset) from the pen and the line's top to the glyph's top-left, xadvance the
 *    pen's step.  The string's bytes are looked up by id (the first match); a byte without a glyph is skipped (GLFont.cpp:597).  width = the sum
 *    of the advances of the bytes that have a glyph.  pen starts at x (CSDR_ALIGN_LEFT), x - floor(width / 2) (_CENTER) or x - width (_RIGHT); the
 *    line's top is y (CSDR_ALIGN_TOP), y - floor(line_height / 2) (_CENTER) or y - line_height (_BOTTOM).  Each glyph with w > 0 and h > 0 gives one
 *    primitive {pen + xoffset, top + yoffset, w, h, rgba, mode, mask x, mask y}.  No scaling and no kerning: the reference stretches every glyph quad
 *    to the line height and widens a space to the aspect of '_' (GLFont.cpp:488-495); that is not reproduced.  More primitives than cap: CSDR_ERANGE
 *    with *n_out the number needed; a halign, valign or mode out of range, a negative w, h or line_height: CSDR_EINVAL. */
#define CSDR_OVL_OVER 0
#define CSDR_OVL_ADD  1
#define CSDR_OVL_COPY 2
typedef struct csdr_overlay_prim {
    int32_t x, y, w, h;        /* tile pixels, row 0 at the top; may lie partly or wholly outside: clipped */
    uint8_t rgba[4];           /* source colour and source alpha a */
    int32_t mode;              /* CSDR_OVL_* */
    int32_t mask_x, mask_y;    /* top-left of a w x h window of the font plane; mask_x < 0: no mask */
} csdr_overlay_prim;
typedef struct csdr_overlay_tile { int32_t first, count; } csdr_overlay_tile;   /* a run of the call's prims; runs may be shared between tiles */
CSDR_STATIC_ASSERT(sizeof(csdr_overlay_prim) == 32 && offsetof(csdr_overlay_prim, rgba) == 16 && offsetof(csdr_overlay_prim, mask_x) == 24 &&
                   sizeof(csdr_overlay_tile) == 8, "csdr_overlay_prim layout");
int  csdr_overlay_create(csdr_ctx *ctx, csdr_overlay **out);
void csdr_overlay_destroy(csdr_overlay *ov);
int  csdr_overlay_setup(csdr_overlay *ov, int max_tiles, int max_prims);
int  csdr_overlay_set_font(csdr_overlay *ov, const uint8_t *a8, int font_w, int font_h);
int  csdr_overlay_compose(csdr_overlay *ov, const uint8_t *base, int base_is_dev, const csdr_overlay_tile *tiles, int n_tiles,
                          const csdr_overlay_prim *prims, int n_prims, int width, int height, int atlas_cols, uint8_t *out_u8, int64_t cap);
int  csdr_overlay_device_view(csdr_overlay *ov, const uint8_t **dev, int *pic_width, int *pic_height);

#define CSDR_ALIGN_LEFT   0    /* halign */
#define CSDR_ALIGN_CENTER 1    /* halign and valign */
#define CSDR_ALIGN_RIGHT  2
#define CSDR_ALIGN_TOP    0    /* valign */
#define CSDR_ALIGN_BOTTOM 2
#define CSDR_SIDEBAND_BOTH 0
#define CSDR_SIDEBAND_USB  1
#define CSDR_SIDEBAND_LSB  2
#define CSDR_MARKER_DELTA_LOCK 1   /* flags of csdr_design_demod_marker */
#define CSDR_MARKER_RECORDING  2
#define CSDR_MARKER_MUTED      4
#define CSDR_MARKER_SOLO       8
#define CSDR_MARKER_CENTERLINE 16
typedef struct csdr_freq_tick { double m, value; int32_t major, column; char label[32]; } csdr_freq_tick;
typedef struct csdr_freq_scale {
    double step_mhz;           /* the visual step: 0.01, 0.1, 0.25 ... 50 */
    double tick_top, label_y;  /* lMhzPos and hPos, NDC */
    int32_t precision;         /* digits of a label: 1, or 2 at the 0.01 step */
    int32_t n_ticks;
    int32_t font_size;         /* 12, or 16 when viewHeight > 135 */
    int32_t tick_rows, label_row;  /* vb(tick_top), vb(label_y) */
    int32_t pad;
} csdr_freq_scale;
typedef struct csdr_db_grid_range { double alpha, step; int32_t first, count; } csdr_db_grid_range;   /* positions p[first .. first + count) */
typedef struct csdr_demod_marker {
    float ux, ofs_left, ofs_right, label_v;   /* uxPos, ofsLeft, ofsRight, hPos */
    int32_t narrow;                           /* ofs * 2 < 16 / viewWidth */
    int32_t halign;                           /* CSDR_ALIGN_* of the label; its valign is CSDR_ALIGN_CENTER */
    int32_t label_x, label_y;                 /* hb(uxPos), vb(hPos) */
    char prefix[8];                           /* "" or "[..] " */
} csdr_demod_marker;
typedef struct csdr_glyph { int32_t id, x, y, w, h, xoffset, yoffset, xadvance; } csdr_glyph;
CSDR_STATIC_ASSERT(sizeof(csdr_freq_tick) == 56 && sizeof(csdr_freq_scale) == 48 && sizeof(csdr_db_grid_range) == 24 && sizeof(csdr_demod_marker) == 40 &&
                   sizeof(csdr_glyph) == 32, "planner record layouts");
int  csdr_design_freq_scale(int64_t freq, int64_t bandwidth, int view_w, int view_h, double font_scale, csdr_freq_scale *out, csdr_freq_tick *ticks, int cap);
int  csdr_design_db_grid(float floor_value, float ceil_value, csdr_db_grid_range *ranges /*[3]*/, int *n_ranges, double *p, int cap);
int  csdr_design_db_labels(float floor_value, float ceil_value, int fft_size, double db_offset, char *ceil_label, char *floor_label, int cap /* bytes of each */);
int  csdr_design_demod_marker(int64_t demod_freq, int bandwidth, int sideband, int64_t center_freq, int64_t srate, int flags, int view_w, int view_h,
                              const uint8_t *rgb /*[3]*/, csdr_demod_marker *out, csdr_overlay_prim *prims /*[4]*/, int *n_prims);
int  csdr_design_text(const csdr_glyph *glyphs, int n_glyphs, int line_height, const char *str, int x, int y, int halign, int valign,
                      const uint8_t *rgba /*[4]*/, int mode, csdr_overlay_prim *out, int cap, int *n_out);

/* ------------------------------------------------------------------ Density bank: spectrum persistence as RGBA tiles
 * The persistence ("digital phosphor") display: for every pixel of a spectrum or scope tile, how often the trace passed through it.  The reference
 * has the idea only as ScopePanel's 0.05-alpha background (src/panel/ScopePanel.cpp:88-89), which "Trace bank" item 4 leaves out.  A csdr_density
 * is a bank of max_slots independent hit grids in HBM, uint32 count[height][width] each, with the tile geometry of csdr_wfbank_render; a step
 * rasterises ALL frames of every listed item -- read where the spectrum, view and scope banks left them in HBM, or given on the host -- and a render
 * maps the counts through a palette.  Every step runs the same two launches and every render the same one launch, whatever the slot, item and
 * frame counts.  THE PICTURE IS THE LIBRARY'S OWN DEFINITION: after the trace bank's one float step per vertex everything is exact integer
 * arithmetic, and every implementation is held to it count for count and byte for byte.
 * 1. Cover of a frame.  A frame is a polyline of n vertices of kind CSDR_TRACE_SPECTRUM or CSDR_TRACE_SCOPE_Y, layout 0 (n y values) or 1 (n (x, y)
 *    pairs).  Its cover is the LINE interval [lo_c, hi_c] of every column c of a tile width x height, exactly as "Trace bank" items 1 - 3 define it:
 *    what csdr_design_trace_envelope(points, NULL, n, layout, kind, width, height, lo, hi) writes into lo[0 .. width) and hi[0 .. width).  The scope's
 *    axis rows are not part of the cover; the other kinds are CSDR_EINVAL.  An item holds `frames` frames, frame f at points + f * stride_floats, and
 *    cover[r][c] is the number of its frames f with lo_c(f) <= r <= hi_c(f).  Rows [0, 9, 0] at width 7, height 10, one frame: cover is 1 exactly on
 *    lo = [0, 2, 7, 2, 0, -, -] .. hi = [2, 7, 9, 7, 2, -, -].
 * 2. Step.  csdr_density_step takes a list of items; for every cell of a slot the list names, evaluated in 64 bits,
 *        count' = min(2^32 - 1, floor(count * keep_q16 / 65536) + weight * cover)
 *    with 0 <= keep_q16 <= 65536 and 1 <= weight <= 2^24.  An item with points == NULL, n == 0 or frames == 0 only decays (cover = 0).  Slots the list
 *    does not name keep their state; a slot named twice in one list is CSDR_EINVAL.  A slot starts all-zero; csdr_density_reset_slot restores that.
 * 3. Peak.  peak[slot] is the maximum count of the slot after its last step (0 for a fresh or reset slot); csdr_density_peak synchronises.
 * 4. Render.  Views {slot, full}; tile k of the atlas is exactly csdr_wfbank_render's (item 6 of "Waterfall bank"): ceil(n_views / atlas_cols) * height
 *    rows by atlas_cols * width pixels, view k at tile row k / atlas_cols, tile column k % atlas_cols.  slot == -1 gives an all-zero tile, and the
 *    unused tiles of the last tile row are all-zero.  Per pixel, with full_eff = full ? full : max(peak[slot], 1):
 *        idx = 0 when count == 0;  idx = 255 when count >= full_eff;  otherwise idx = max(1, floor(count * 255 / full_eff)), in 64 bits
 *    and the four bytes of the pixel are palette[idx].  csdr_density_set_palette sets the 256 x RGBA palette, one per object; before any call it is
 *    (i, i, i, 255).  A cell that was hit is never drawn with index 0.  out_u8 == NULL leaves the picture on the device; csdr_density_device_view
 *    returns the last rendered picture and its size in pixels with the trace bank's rules (valid until the next render or setup), so a csdr_overlay
 *    takes it as its base.
 * 5. Readers in HBM.  csdr_density_step_spec steps `slot` with frames [frame0, frame0 + n_frames) of a spectrum's last process as ONE item of kind
 *    CSDR_TRACE_SPECTRUM with n = the spectrum's fftSize: vertex i of a frame is the point csdr_spec_fetch would return at i, the DC-spike overwrite
 *    of csdr_spec_set_hide_dc included.  csdr_density_step_specbank steps slot s with the csdr_specbank_frames(sb, s) frames of slot s of a
 *    spectrum bank's last process, for every s below the smaller of the two slot counts (a slot without frames only decays), n = the bank's fftSize.  Both
 *    order themselves against the producer by events, as csdr_waterfall_step_spec and csdr_wfbank_step_specbank do: nothing waits on the host and
 *    the producer's next process waits for the reads.  View-bank and scope-bank points come in as items with is_dev = 1, from
 *    csdr_viewbank_device_points / csdr_scopebank_device_points.
 * 6. Limits.  2 <= width <= 16384, 1 <= height <= 2048, max_slots >= 1 and max_slots * height * width <= 2^30, 1 <= max_frames <= 2^20,
 *    1 <= max_points <= 2^21, 1 <= n_items <= max_slots, 1 <= atlas_cols <= n_views <= 2^20.  A kind other than the two, a layout other than 0 | 1,
 *    n < 0, frames < 0, is_dev other than 0 | 1, a slot out of range or named twice, stride_floats below n * (1 + layout) where frames are read,
 *    keep_q16 above 65536, weight 0 or above 2^24, device points that are not 4-byte aligned: CSDR_EINVAL.  frames above max_frames, n above
 *    max_points, a host buffer too small: CSDR_ERANGE.  A refusal changes nothing.
 * 7. csdr_design_density_cover is item 1 on the host, no device needed: cover[height][width], uint32, is overwritten.
 * Ordering is the trace bank's.  All work runs on a stream of the object's own; csdr_density_fetch, csdr_density_peak and a render into host memory
 * synchronise it.  Host points are copied into page-locked staging inside the call, so the caller's buffers are free when it returns.  Device points
 * must have been produced on, or handed to, the boundary stream -- what csdr_specbank_device_points, csdr_viewbank_device_points and
 * csdr_scopebank_device_points do -- are ordered behind it by an event and stay unchanged until the next synchronising call on this object.
 * csdr_density_device_view makes the boundary stream wait for the picture.  The producing banks are not touched and wait for nobody here: a caller
 * who steps from device points synchronises this object -- csdr_density_fetch, csdr_density_peak or a render into host memory -- before the
 * producer's next process, the rule those device_points calls give every reader.  A call waits on the host only for the upload of its records that
 * last used the same page-locked staging set, two calls ago. */
typedef struct csdr_density_item {
    const float *points;       /* the frames' vertices; NULL: the slot only decays */
    int64_t stride_floats;     /* from the first float of a frame to the first float of the next; >= n * (1 + layout) */
    int32_t slot;              /* the slot the item updates */
    int32_t n;                 /* vertices per frame; 0: the slot only decays */
    int32_t frames;            /* frames; 0: the slot only decays */
    int32_t layout;            /* 0: y values; 1: (x, y) pairs */
    int32_t kind;              /* CSDR_TRACE_SPECTRUM | CSDR_TRACE_SCOPE_Y */
    int32_t is_dev;            /* 1: `points` is device memory, 4-byte aligned */
    uint32_t keep_q16;         /* decay factor, 0 .. 65536 */
    uint32_t weight;           /* hits one frame adds, 1 .. 2^24 */
} csdr_density_item;
CSDR_STATIC_ASSERT(sizeof(csdr_density_item) == 48 && offsetof(csdr_density_item, stride_floats) == 8 && offsetof(csdr_density_item, slot) == 16 &&
                   offsetof(csdr_density_item, is_dev) == 36 && offsetof(csdr_density_item, weight) == 44, "csdr_density_item layout");
typedef struct csdr_density_view {
    int32_t slot;              /* -1: an all-zero tile */
    uint32_t full;             /* the count drawn with palette[255]; 0: the slot's peak */
} csdr_density_view;
CSDR_STATIC_ASSERT(sizeof(csdr_density_view) == 8 && offsetof(csdr_density_view, full) == 4, "csdr_density_view layout");
int  csdr_density_create(csdr_ctx *ctx, csdr_density **out);
void csdr_density_destroy(csdr_density *db);
int  csdr_density_setup(csdr_density *db, int width, int height, int max_slots, int max_frames, int max_points);     /* every slot all-zero */
int  csdr_density_set_palette(csdr_density *db, const uint8_t *rgba /*[256][4]*/);
int  csdr_density_reset_slot(csdr_density *db, int slot);
int  csdr_density_step(csdr_density *db, const csdr_density_item *items, int n_items);
int  csdr_density_step_spec(csdr_density *db, int slot, csdr_spec *spec, int frame0, int n_frames, uint32_t keep_q16, uint32_t weight);
int  csdr_density_step_specbank(csdr_density *db, csdr_specbank *sb, uint32_t keep_q16, uint32_t weight);
int  csdr_density_peak(csdr_density *db, int slot, uint32_t *peak);
int  csdr_density_fetch(csdr_density *db, int slot, uint32_t *out /*[height][width]*/, int64_t cap /* entries */);
int  csdr_density_render(csdr_density *db, const csdr_density_view *views, int n_views, int atlas_cols, uint8_t *out_u8, int64_t cap);
int  csdr_density_device_view(csdr_density *db, const uint8_t **dev, int *pic_width, int *pic_height);
int  csdr_design_density_cover(const float *points, int n, int layout, int64_t stride_floats, int frames, int kind, int width, int height,
                               uint32_t *cover /*[height][width]*/);

/* ------------------------------------------------------------------ ingest
 * The reference's reader fills pooled SDRThreadIQData blocks (SoapySDRThread.cpp:221-225) and SDRPostThread hands ONE buffer to the
 * demodulator and the visual queues (SDRPostThread.cpp:227-245).  Here the reader fills a page-locked slot in place, commit moves it
 * over the link ONCE on a transfer stream of its own (optionally exchanging I and Q on the way: the iq_swap option of
 * SoapySDRThread.cpp:258-266) and returns the device pointer every consumer reads (csdr_post_execute / csdr_spec_process with
 * iq_is_dev = 1); it stays valid until `depth - 1` further commits.  Slot k + 1 crosses the link while slot k is processed. */
int  csdr_ingest_create(csdr_ctx *ctx, int64_t max_samples, int depth, csdr_ingest **out);
void csdr_ingest_destroy(csdr_ingest *ing);
int  csdr_ingest_acquire(csdr_ingest *ing, float **host_slot);
int  csdr_ingest_commit(csdr_ingest *ing, int64_t n_samples, int iq_swap, const float **dev_iq);
/* the same single transfer for a block assembled in the caller's own memory (pooled SDRThreadIQData blocks, page-locked once with
 * csdr_host_register); waits for the previous upload first.  csdr_ingest_next_slot: the ring slot the next transfer will overwrite. */
int  csdr_ingest_upload(csdr_ingest *ing, const float *host_iq, int64_t n_samples, int iq_swap, const float **dev_iq);
int  csdr_ingest_next_slot(const csdr_ingest *ing);
int  csdr_ingest_wait(csdr_ingest *ing);             /* blocks until the last transfer has left its source buffer: call before rewriting or recycling the block just uploaded */

/* ------------------------------------------------------------------ ingest of a radio's native sample format
 * Receivers deliver 8-, 12- or 16-bit integers (SoapySDR's "CU8", "CS8", "CS12", "CS16", with the full scale getNativeStreamFormat reports); the
 * reference asks the driver for "CF32" (SoapySDRThread.cpp:88-90), so the widening runs sample by sample on a host core before readStream
 * (:253, :294-308) sees the data.  A raw ingest carries the radio's own bytes over the link -- 4, 3 or 2 per sample instead of 8 -- in page-locked
 * slots of that size, and widens them on the GPU into the same CF32 ring in HBM that every consumer reads.
 *
 * A sample is a pair (I, Q), little-endian:
 *   CSDR_IQ_CF32  8 bytes  float I, float Q       (accepted so that callers have one code path: no conversion runs, full_scale / offset are unused)
 *   CSDR_IQ_CS16  4 bytes  int16 I, int16 Q
 *   CSDR_IQ_CS8   2 bytes  int8 I, int8 Q
 *   CSDR_IQ_CU8   2 bytes  uint8 I, uint8 Q       (offset binary)
 *   CSDR_IQ_CS12  3 bytes  b0 = I[7:0], b1 = Q[3:0] << 4 | I[11:8], b2 = Q[11:4]; both sign-extended from 12 bits
 * THE ARITHMETIC, which the device kernel, the host mirror's fall-back and the tests' restatement share bit for bit: every component is
 *     y = ((float)x - offset) * s,    s = (float)(1.0 / full_scale)
 * with s rounded once on the host, the subtraction and the product each rounded once in float32 and never contracted into one operation
 * ((float)x is exact for all these widths).  With iq_swap the two CONVERTED components change places.  This is the library's own definition:
 * it is not claimed to equal any particular driver's host conversion.
 * Refused with CSDR_EINVAL: an unknown format, a full_scale that is not finite and positive, a non-finite offset, a non-zero offset with a
 * signed format (offset is the caller's choice for CU8: 128, 127.5, or the 127.4 some RTL-SDR drivers use). */
#define CSDR_IQ_CF32 0
#define CSDR_IQ_CS16 1
#define CSDR_IQ_CS8  2
#define CSDR_IQ_CU8  3
#define CSDR_IQ_CS12 4
typedef struct csdr_iq_format {
    int32_t format;            /* CSDR_IQ_* */
    float   offset;            /* subtracted from (float)x: 0 for the signed formats */
    double  full_scale;        /* 32768, 2048, 128 ...: y = 1 at x - offset = full_scale */
} csdr_iq_format;
CSDR_STATIC_ASSERT(sizeof(csdr_iq_format) == 16 && offsetof(csdr_iq_format, full_scale) == 8, "csdr_iq_format layout");
/* bytes n_samples samples occupy in `format` */
int  csdr_iq_format_bytes(int format, int64_t n_samples, uint64_t *bytes);
/* A ring like csdr_ingest_create's whose page-locked slots hold max_samples samples of *fmt (csdr_iq_format_bytes, not 8 * max_samples); the HBM
 * ring, the events and the lifetime of the returned device pointer (valid until depth - 1 further commits) are the same.  acquire_raw gives the slot
 * the reader fills with the radio's bytes; commit_raw moves its first n_samples over the link as they are -- ONE DMA into a staging buffer in HBM that
 * the ingest owns -- and converts them into the HBM slot behind it, both on the ingest's transfer stream.  (The converting kernel reading the mapped
 * slot over the link, as the exchanging commit of the typed ring does, was measured too: slower beside a running pipeline) */
int  csdr_ingest_create_raw(csdr_ctx *ctx, int64_t max_samples, int depth, const csdr_iq_format *fmt, csdr_ingest **out);
int  csdr_ingest_acquire_raw(csdr_ingest *ing, void **host_slot);
int  csdr_ingest_commit_raw(csdr_ingest *ing, int64_t n_samples, int iq_swap, const float **dev_iq);
/* the same for a block in the caller's own memory (page-locked with csdr_host_register or pageable, any alignment): ONE hipMemcpyAsync of the raw
 * bytes into the same staging buffer (allocated on first use), then the conversion in HBM, both on the transfer stream.  The previous upload is
 * waited for first, as in csdr_ingest_upload. */
int  csdr_ingest_upload_raw(csdr_ingest *ing, const void *host_raw, int64_t n_samples, int iq_swap, const float **dev_iq);
/* change full_scale / offset, or switch to a format whose samples are no larger than those the ring was created for, between blocks: takes effect at
 * the next commit / upload (what is already enqueued keeps the format it was enqueued with) */
int  csdr_ingest_set_format(csdr_ingest *ing, const csdr_iq_format *fmt);
/* the conversion kernel alone, for parity checks: n_samples of *fmt at raw_host -> out_host[2 * n_samples] floats */
int  csdr_iq_convert(csdr_ctx *ctx, const csdr_iq_format *fmt, const void *raw_host, int64_t n_samples, int iq_swap, float *out_host);
/* The typed calls (csdr_ingest_acquire / _commit / _upload) on a raw ingest and the raw calls on a typed one return CSDR_ESTATE (a raw ingest whose
 * format is CSDR_IQ_CF32 is still a raw ingest: its slots are reached through the raw calls); n_samples beyond the slot is CSDR_ERANGE.  Every
 * refusal enqueues nothing and leaves the ring where it was. */

/* ------------------------------------------------------------------ one stream over several GPUs
 * Replaces the fan-out point SDRPostThread.cpp:389-396 (one block pushed to every demodulator's queue) when the DemodulatorInstances
 * of ONE stream are spread over the GPUs of a node: one process per GPU, each with its own csdr_ctx.  Rank 0 makes the 128-byte id
 * (csdr_comm_unique_id) and the HOST hands it to every rank (pipe, socket, MPI ...); csdr_comm_create is collective.  Every call below
 * is collective too and is enqueued on the context's boundary stream: behind all the library's earlier work on this context, and the
 * library's next work starts behind it -- no host synchronisation on the data path.  RCCL is loaded on first use (dlopen): a
 * single-GPU user never maps it.  Buffers are device memory; counts are complex samples.
 *   broadcast     the ingest rank's raw IQ batch (then csdr_post_set_active_channels + csdr_post_execute on every rank: SURVEY 8e option 1)
 *   scatter       root holds world x n_samples (rank r's part at 2 * r * n_samples floats); every rank receives its part (time slabs)
 *   all_to_all    send_samples[q] to rank q, recv_samples[p] from rank p, consecutive in the buffers: one send / receive per xGMI peer pair
 *   max           max over the ranks of a host scalar; also a barrier (returns when this rank's enqueued work is done and all ranks arrived)
 *   csdr_post_exchange_rows  one batch of the time-slab variant: export of the rows every peer owns from `producer` (which has just
 *                 executed this rank's blocks for all channels), all-to-all, import into `owner` at each peer's frame offset, commit.
 *                 channels: the ranks' channel lists one after the other (n_channels[q] entries for rank q); frame0 / frames [world]. */
#define CSDR_COMM_ID_BYTES 128
/* Errors.  Every entry point validates its arguments and allocates before the first call the peers take part in, so a refused call (CSDR_EINVAL,
 * CSDR_ENOMEM, CSDR_ESTATE) has enqueued nothing and the communicator stays usable -- provided EVERY rank is refused alike: the ranks of one
 * collective must pass consistent arguments (the same channel lists and row order in csdr_post_exchange_rows; whether the producers' rows
 * travel as they lie is decided from the producer's row order, which therefore has to be the same on every rank).  A rank that fails INSIDE a
 * collective (CSDR_EHIP after its peers may have entered the matching calls) aborts its communicators (ncclCommAbort): its connections are torn
 * down, so the peers' pending transfers end with an error instead of waiting for good -- they see it through csdr_comm_async_error (poll it where
 * the host would otherwise block on the stream), which aborts theirs too.  An aborted communicator refuses every later call (CSDR_ESTATE): destroy
 * it on every rank and make a new one.  csdr_comm_abort does the same on request (a rank that must leave for a reason of its own). */
int  csdr_comm_unique_id(char *id_out /* [CSDR_COMM_ID_BYTES] */);
int  csdr_comm_create(csdr_ctx *ctx, const char *unique_id, int rank, int world, csdr_comm **out);
void csdr_comm_destroy(csdr_comm *comm);
int  csdr_comm_rank(const csdr_comm *comm);
int  csdr_comm_world(const csdr_comm *comm);
int  csdr_comm_broadcast(csdr_comm *comm, float *iq_dev, int64_t n_samples, int root);
int  csdr_comm_scatter(csdr_comm *comm, const float *send_dev, float *recv_dev, int64_t n_samples, int root);
int  csdr_comm_all_to_all(csdr_comm *comm, const float *send_dev, const int64_t *send_samples, float *recv_dev, const int64_t *recv_samples);
typedef struct csdr_p2p_op { int32_t peer; int32_t recv; float *buf; int64_t n_samples; } csdr_p2p_op;
/* n point-to-point transfers as one group (a scatter of overlapping windows, any irregular exchange): op i sends n_samples from buf to peer
 * (recv == 0) or receives them into buf; peer == this rank is refused (a rank's own part needs no transfer) */
int  csdr_comm_p2p(csdr_comm *comm, const csdr_p2p_op *ops, int n);
int  csdr_comm_max(csdr_comm *comm, double *value);
int  csdr_comm_barrier(csdr_comm *comm);
int  csdr_post_exchange_rows(csdr_comm *comm, csdr_post *producer, csdr_post *owner, const int *channels, const int *n_channels,
                             const int64_t *frame0, const int64_t *frames, int n_blocks, int block_len, int64_t frequency);
/* The same exchange in two halves, so that the transfers of batch i run beside the channelizer of batch i + 1 (SDRPostThread.cpp:389-396 hands a
 * block to the demodulators' queues and goes straight on to the next one: the queue is the overlap there).  Host order per batch:
 *     csdr_post_execute(producer, batch i + 1);  _begin(...batch i + 1...);  _finish(owner, batch i);  csdr_bank_execute(bank, owner);
 *   _begin   enqueues the grouped sends / receives on the communicator's own transfer stream (and, where RCCL can split one off, its own
 *            communicator), behind the producer's kernels only; no lane of the library waits for them.  From its first _begin on, the producer
 *            rotates its output buffers whatever the stream folding and rewrites a buffer only behind the transfers that read it.
 *   _finish  the oldest batch begun and not finished: the owner's lane waits for that batch's transfers, imports and commits (n_blocks,
 *            block_len, frequency describe THAT batch).
 * At most two batches may be between their halves (CSDR_ESTATE beyond); csdr_comm_exchanges_pending counts them.  The owner's rows -- and the
 * audio behind them -- equal the one-call form's bit for bit. */
int  csdr_post_exchange_rows_begin(csdr_comm *comm, csdr_post *producer, const int *channels, const int *n_channels,
                                   const int64_t *frame0, const int64_t *frames);
int  csdr_post_exchange_rows_finish(csdr_comm *comm, csdr_post *owner, int n_blocks, int block_len, int64_t frequency);
int  csdr_comm_exchanges_pending(const csdr_comm *comm);
int  csdr_comm_abort(csdr_comm *comm);
int  csdr_comm_async_error(csdr_comm *comm);        /* CSDR_OK: no transfer of this communicator has failed; otherwise it has been aborted here too */

#ifdef __cplusplus
}
#endif
#endif /* CSDR_HIP_H */
