"""-m gpu parity tests: the HIP path (through the C ABI) against the reference's own liquid-dsp 1.5.0 binary
(oracle backend "ref" when oracle/_ref/libliquid.dll travelled to the box, else the pinned C restatement "port").

Tolerances (BASELINE.json north_star): integer items (per-block output counts, NCO phase word, resampler phase,
half-band buffer fill) bit-exact; float32 samples within 1e-5 of the reference's peak magnitude.
"""
import numpy as np
import pytest

from tests.util import demod_frequencies, exact_spectrum, rel_err, synth_iq, synth_iq_fast

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _backend():
    import oracle.liquid_api as A
    return "ref" if A.available("ref") else "port"


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------------------------- SDRPostThread
@pytest.mark.parametrize("fs,M,block", [(2400000, 4, 40000), (10000000, 20, 166680), (3000000, 6, 50004), (1000000, 2, 16668)])
def test_channelizer_matches_firpfbch(ctx, fs, M, block):
    from cubicsdr_amd.engine import SDRPost
    from oracle.cubicsdr_chain import RefSDRPost
    center = 100000000
    x = [synth_iq(block, fs, center, [("NBFM", center + 123456)], seed=11 + b, t0=b * block) for b in range(3)]
    ref = RefSDRPost(_backend(), fs, M)
    post = SDRPost(ctx, fs, M, block, max_blocks=1)
    for b in range(3):
        ref.run_block(x[b], center)
        post.execute(x[b], 1, block, center)
        for ch in range(M + 1):
            want, fc, rate = ref.channel_data(ch)
            got = post.read_channel(ch)
            assert post.channel_center(ch) == fc
            assert rel_err(got, want) < TOL, (b, ch)
        assert post.channel_bandwidth == ref.chan_bw
    for f in (center, center + 123456, center - fs // 2 + 1, center + fs // 2 - 1, center + 3 * (fs // M) + 7):
        assert post.channel_at(f) == ref.channel_at(f)
    post.close()


@pytest.mark.parametrize("fs,M,block", [(2400000, 4, 40000), (10000000, 20, 166680), (3000000, 6, 50004), (61440000, 122, 102480),
                                         (100000000, 1024, 65536), (1000000, 2, 16668),
                                         # round 5: the oversampled hop inside the FFT channelizer (M % 4 == 0 and a 16-frame tile fits): whole and ragged tiles, one to
                                         # three passes, a wide-odd factor, blocks shorter than a tile
                                         (4000000, 8, 8 * 517), (20000000, 40, 40 * 301), (100000000, 200, 200 * 77), (128000000, 256, 256 * 53),
                                         (34000000, 68, 68 * 45), (56000000, 112, 112 * 5),
                                         # round 6: M / 2 odd on chan_analyze_p2 (ragged tiles, a block shorter than a tile, the first and the last count of the range)
                                         (61440000, 122, 122 * 77), (61440000, 122, 122 * 9), (33000000, 66, 66 * 100), (63000000, 126, 126 * 65), (19000000, 38, 38 * 130), (17000000, 34, 34 * 130)])
def test_channelizer2_matches_firpfbch2(ctx, fs, M, block):
    """SDRPostPFBCH2 (runPFBCH2, SDRPostThread.cpp:472-512): firpfbch2 hands out M samples per M/2 inputs, every channel at
    twice the channel spacing; M/2 odd (6, 122) starts every other frame at an odd sample offset; M = 1024 takes the
    unstaged kernel variant.  Three blocks one at a time (carried history), then the same three in one batch."""
    from cubicsdr_amd.engine import SDRPost
    from oracle.cubicsdr_chain import RefSDRPost
    center = 100000000
    x = [synth_iq(block, fs, center, [("NBFM", center + 123456)], seed=41 + b, t0=b * block) for b in range(3)]
    ref = RefSDRPost(_backend(), fs, M, oversampled=True)
    post = SDRPost(ctx, fs, M, block, max_blocks=1, oversampled=True)
    # (round 6: M / 2 odd from M = 38 on -- the 61.44 MS/s count 122 among them -- runs the matrix-pipe form of chan_analyze_p2, the two lattices of frames dealt to its waves)
    want_kernel = "chan_analyze_fft" if M % 4 == 0 and M < 1024 else "chan_analyze_p2" if (M // 2) % 2 == 1 and 38 <= M <= 126 else "chan_analyze"
    assert post.kernel_name == want_kernel, post.kernel_name
    chans = range(M + 1) if M <= 122 else sorted({c for c in (0, 1, 2, M // 2 - 1, M // 2, M // 2 + 1, M - 1, M, 77, 511, 512, 513, 1023, 1024) if c <= M})
    want_all = {ch: [] for ch in chans}
    for b in range(3):
        ref.run_block(x[b], center)
        post.execute(x[b], 1, block, center)
        peak = float(np.max(np.abs(ref.data_out)))              # tolerance relative to the strongest channel of the block
        for ch in chans:
            want, fc, rate = ref.channel_data(ch)
            got = post.read_channel(ch)
            assert got.size == want.size == 2 * block // M
            assert post.channel_center(ch) == fc and post.channel_rate == rate == 2 * (fs // M)
            noise = 4 * np.spacing(np.float32(0.01 * M / 0.0005)) if ch == 0 else 0.0     # DC-blocker state noise (see C4 test)
            assert np.max(np.abs(got - want)) < TOL * peak + noise, (b, ch)
            want_all[ch].append(want)
    assert post.channel_bandwidth == ref.chan_bw
    post.close()
    batch = SDRPost(ctx, fs, M, block, max_blocks=3, oversampled=True)
    batch.execute(np.concatenate(x), 3, block, center)
    peak = max(float(np.max(np.abs(np.concatenate(want_all[ch])))) for ch in chans)
    for ch in chans:
        want = np.concatenate(want_all[ch])
        noise = 4 * np.spacing(np.float32(0.01 * M / 0.0005)) if ch == 0 else 0.0
        assert np.max(np.abs(batch.read_channel(ch) - want)) < TOL * peak + noise, ch
    batch.close()


def _channelizer_case(ctx, fs, M, block, chans=None, nblocks=3):
    """`nblocks` blocks one at a time (carried history), then the same blocks in one batch, every channel (or `chans`) against the
    reference's firpfbch.  Tolerance relative to the strongest channel of the block (a DFT's rounding error scales with the frame's
    energy; the reference's own mixed-radix / Rader FFT is no closer to the exact transform in the quiet channels)."""
    from cubicsdr_amd.engine import SDRPost
    from oracle.cubicsdr_chain import RefSDRPost
    center = 100000000
    x = [synth_iq(block, fs, center, [("NBFM", center + 123456), ("AM", center - 7 * (fs // M) + 999)], seed=71 + b, t0=b * block) for b in range(nblocks)]
    ref = RefSDRPost(_backend(), fs, M)
    post = SDRPost(ctx, fs, M, block, max_blocks=1)
    chans = list(range(M + 1)) if chans is None else list(chans)
    want_all = {ch: [] for ch in chans}
    worst = 0.0
    for b in range(nblocks):
        ref.run_block(x[b], center)
        post.execute(x[b], 1, block, center)
        peak = float(np.max(np.abs(ref.data_out)))
        for ch in chans:
            want, fc, rate = ref.channel_data(ch)
            got = post.read_channel(ch)
            assert got.size == want.size == block // M
            assert post.channel_center(ch) == fc
            noise = 4 * np.spacing(np.float32(0.01 * M / 0.0005)) if ch == 0 else 0.0     # DC-blocker state noise (see C4 test)
            err = float(np.max(np.abs(got - want)))
            assert err < TOL * peak + noise, (b, ch, err / peak)
            if ch:
                worst = max(worst, err / peak)
            want_all[ch].append(want)
    post.close()
    batch = SDRPost(ctx, fs, M, block, max_blocks=nblocks)
    batch.execute(np.concatenate(x), nblocks, block, center)
    peak = max(float(np.max(np.abs(np.concatenate(want_all[ch])))) for ch in chans)
    for ch in chans:
        want = np.concatenate(want_all[ch])
        noise = 4 * np.spacing(np.float32(0.01 * M / 0.0005)) if ch == 0 else 0.0
        assert np.max(np.abs(batch.read_channel(ch) - want)) < TOL * peak + noise, ch
    batch.close()
    return worst


@pytest.mark.parametrize("fs,M,block", [(5000000, 10, 83340), (7000000, 14, 14 * 70), (61440000, 122, 122 * 150), (61440000, 122, 1024068),
                                        (37000000, 74, 74 * 150), (47000000, 94, 94 * 97), (59000000, 118, 118 * 131), (31000000, 62, 62 * 140), (11000000, 22, 22 * 300)])
def test_channelizer_m_twice_odd(ctx, fs, M, block):
    """M = 2 A with A an odd prime (10, 14, 122 = the 61.44 MS/s channel count, SoapySDRThread.cpp:676-693) runs the one-lane-per-frame
    kernel (chan_analyze_p2): whole and ragged 64-frame tiles.  From A = 11 (M = 22) on its transform phase runs on the matrix pipe: one row tile of
    outputs up to M = 62, two from M = 74 (three outputs in the second tile; 94, 118, 122: 31 of the 32 outputs and terms in use); M = 10 / 14 are the
    vector form."""
    from cubicsdr_amd.engine import SDRPost
    probe = SDRPost(ctx, fs, M, block)
    assert probe.kernel_name == "chan_analyze_p2", probe.kernel_name
    probe.close()
    _channelizer_case(ctx, fs, M, block)


# (M, frames per block): every butterfly of chan_analyze_fft (16 / 8 / 4 / 2, 3 / 5 / 7 / 9 / 11 / 13), one to four passes, tiles of 16 .. 256
# frames whole and ragged, blocks shorter than one tile and shorter than the FIR's reach; 68 = 4 * 17, 76 = 4 * 19, 92 = 4 * 23, 136, 204 = 12 * 17: the wide-odd
# instance (round 5); 116 = 4 * 29 and 2048 (no 8-frame tile in 160 KB) stay on chan_analyze
FFT_SIZES = [(2, 700), (4, 1000), (8, 515), (12, 300), (16, 260), (20, 777), (24, 130), (28, 100), (36, 70), (40, 300), (44, 65), (52, 40), (56, 66),
             (72, 50), (80, 129), (100, 90), (112, 33), (126 * 2, 20), (200, 100), (256, 37), (360, 20), (1024, 40), (2048, 19), (68, 30), (32, 5), (200, 3),
             (76, 45), (92, 33), (136, 40), (204, 25), (116, 21), (134, 20), (146, 19), (202, 18), (398, 17), (174, 20), (194, 16), (388, 12), (254, 14), (326, 13), (232, 16), (290, 12), (348, 10), (178, 19), (356, 9), (422, 9), (446, 8)]


@pytest.mark.parametrize("M,frames", FFT_SIZES)
def test_channelizer_fft_sizes(ctx, M, frames):
    """SDRPostThread::runPFBCH (SDRPostThread.cpp:416-455) for the channel counts getOptimalChannelCount can return
    (SoapySDRThread.cpp:676-693: any even number): mixed-radix FFT kernel against the reference's firpfbch_crcf."""
    chans = None if M <= 256 else sorted({c for c in (0, 1, 2, 3, M // 4 - 1, M // 4, M // 2 - 1, M // 2, M // 2 + 1, M - 2, M - 1, M, 77, 500, 333) if c <= M})
    from cubicsdr_amd.engine import SDRPost
    probe = SDRPost(ctx, 500000 * M, M, M * frames)
    # (round 6: a prime factor 29 .. 199 -- 116, 134, 174 ... 398 -- takes the direct prime pass of the FFT kernel, on the fp32 matrix pipe; one >= 211 -- 422, 446 -- its chirp-z pass)
    assert probe.kernel_name == ("chan_analyze" if M == 2048 else "chan_analyze_fft"), probe.kernel_name
    probe.close()
    _channelizer_case(ctx, 500000 * M, M, M * frames, chans=chans)


def test_every_even_channel_count_up_to_400_takes_a_fast_kernel(ctx):
    """getOptimalChannelCount (SoapySDRThread.cpp:676-693) returns any even number: every one of the 200 up to 400 runs the FFT channelizer or, for
    M = 2 x odd <= 126, chan_analyze_p2 -- since round 6 also the 64 counts with a prime factor >= 29 (direct prime pass below 97, chirp-z pass from there)"""
    from cubicsdr_amd.engine import SDRPost
    slow = []
    for M in range(2, 401, 2):
        probe = SDRPost(ctx, 500000 * M, M, M * 16)
        if probe.kernel_name not in ("chan_analyze_fft", "chan_analyze_p2"):
            slow.append((M, probe.kernel_name))
        probe.close()
    assert not slow, slow


@pytest.mark.parametrize("fs,M,block", [(2400000, 4, 40000), (61440000, 122, 122 * 70), (61440000, 122, 122 * 3), (59000000, 118, 118 * 129)])
def test_channelizer_batched_equals_blockwise(ctx, fs, M, block):
    """one call over four blocks = four calls over one block each, bit for bit: the carried history, tiles that end inside a block (M = 122 / 126: the
    matrix-pipe form of chan_analyze_p2 at M = 122 / 118, 64-frame tiles over 70-, 3- and 129-frame blocks -- a block shorter than the FIR's reach included)"""
    from cubicsdr_amd.engine import SDRPost
    center = 100000000
    x = synth_iq(4 * block, fs, center, [("NBFM", center + 200000)], seed=5)
    a = SDRPost(ctx, fs, M, block, max_blocks=4)
    a.execute(x, 4, block, center)
    b2 = SDRPost(ctx, fs, M, block, max_blocks=1)
    outs = [[] for _ in range(M)]
    for k in range(4):
        b2.execute(x[k * block:(k + 1) * block], 1, block, center)
        for ch in range(M):
            outs[ch].append(b2.read_channel(ch))
    for ch in range(M):
        assert np.array_equal(a.read_channel(ch), np.concatenate(outs[ch])), ch
    a.close(); b2.close()


def test_single_channel_dc_blocker(ctx):
    from cubicsdr_amd.engine import SDRPost
    from oracle.cubicsdr_chain import RefSDRPost
    fs, block, center = 480000, 8000, 50000000
    ref = RefSDRPost(_backend(), fs, 1)
    post = SDRPost(ctx, fs, 1, block, max_blocks=1)
    for b in range(4):
        x = synth_iq(block, fs, center, [("NBFM", center + 50000)], seed=21 + b, t0=b * block)
        ref.run_block(x, center)
        post.execute(x, 1, block, center)
        assert rel_err(post.read_channel(0), ref.data_out) < TOL, b
    post.close()


def test_dc_blocker_large_offset_state_noise(ctx):
    """With a large DC offset the reference's float32 recurrence state v ~ DC / 0.0005 carries rounding noise of
    ~ulp(v) per sample that no re-ordering reproduces (the GPU evaluates the recurrence exactly, in fp64): the two
    must agree to that noise floor."""
    from cubicsdr_amd.engine import SDRPost
    from oracle.cubicsdr_chain import RefSDRPost
    fs, block, center = 480000, 8000, 50000000
    ref = RefSDRPost(_backend(), fs, 1)
    post = SDRPost(ctx, fs, 1, block, max_blocks=1)
    dc = (0.05, -0.02)
    v_scale = max(abs(dc[0]), abs(dc[1])) / 0.0005
    noise_floor = 4 * np.spacing(np.float32(v_scale))
    for b in range(4):
        x = synth_iq(block, fs, center, [("NBFM", center + 50000)], seed=21 + b, t0=b * block, dc=dc)
        ref.run_block(x, center)
        post.execute(x, 1, block, center)
        got, want = post.read_channel(0), ref.data_out
        assert np.max(np.abs(got - want)) < TOL * np.max(np.abs(want)) + noise_floor, b
    post.close()


# ----------------------------------------------------------------------------------------------- demodulators
def _gpu_demods(ctx, x, fs, M, block, demods, bws, n_blocks, batch, oversampled=False):
    """the HIP path over n_blocks blocks of x in batches of `batch`: per demodulator the list of per-block results"""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    center = 100000000
    post = SDRPost(ctx, fs, M, block, max_blocks=batch, oversampled=oversampled)
    bank = DemodBank(ctx, len(demods), max_blocks=batch)
    for i, (k, f) in enumerate(demods):
        bank.configure(i, post, k, bws[i], f)
    got = [[] for _ in demods]
    for b0 in range(0, n_blocks, batch):
        post.execute(x[b0 * block:(b0 + batch) * block], batch, block, center)
        bank.execute(post)
        for i in range(len(demods)):
            res = bank.results(i)
            audio = bank.audio(i)
            iq = bank.iq(i)
            o = 0
            for r in res:
                got[i].append(dict(n_iq=r.n_iq, n_audio=r.n_audio, audio=audio[r.audio_offset:r.audio_offset + r.n_audio],
                                   iq=iq[o:o + r.n_iq], level_accum=r.level_accum, level_count=r.level_count, peak=r.audio_peak,
                                   skipped=r.skipped, nco_theta=r.nco_theta, resamp_phase=r.resamp_phase, buffer_index=r.buffer_index))
                o += r.n_iq
    post.close(); bank.close()
    return got


def _ref_demods(x, fs, M, block, demods, bws, n_blocks, oversampled=False, modem_iq=None):
    """the reference path block by block.  modem_iq: {slot: list of per-block IQ arrays} fed to that slot's MODEM instead of the
    reference front-end's own IQ (which is still produced and compared)."""
    from oracle.cubicsdr_chain import RefDemod, RefSDRPost
    center = 100000000
    be = _backend()
    ref_post = RefSDRPost(be, fs, M, oversampled=oversampled)
    def make(i):
        return RefDemod(be, demods[i][0], bws[i], demods[i][1], ref_post.chan_bw * (2 if oversampled and M > 1 else 1))
    if len(demods) > 64:
        # liquid designs every resampler from scratch (0.3 s per demodulator through the reference binary): the full-size configurations
        # build their hundreds of independent objects on a thread pool (the calls release the GIL)
        import os
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max(1, min(32, (os.cpu_count() or 2) - 1))) as ex:
            refs = list(ex.map(make, range(len(demods))))
    else:
        refs = [make(i) for i in range(len(demods))]
    # where the reference's own modem classes were built (oracle/_ref/libref_modems.so: src/modules/modem/analog/Modem*.cpp, unmodified),
    # every block also goes through them: the Python glue the comparison uses must reproduce their audio bit for bit on THIS signal
    cpp = None
    if be == "ref" and len(demods) <= 64:
        from oracle import ref_modems as RM
        if RM.available():
            cpp = [RM.RefModem(k, bws[i]) for i, (k, f) in enumerate(demods)]
    want = [[] for _ in demods]
    _ref_demods.last_channels = [None] * len(demods)          # the channel each demodulator was routed to (for the callers that ask)
    for b in range(n_blocks):
        ref_post.run_block(x[b * block:(b + 1) * block], center)
        chan_cache = {}       # one buffer per channel per block, shared by its demods (SDRPostThread.cpp:341-396)
        for i, rd in enumerate(refs):
            ch = ref_post.channel_at(rd.frequency)
            _ref_demods.last_channels[i] = ch
            if ch not in chan_cache:
                chan_cache[ch] = ref_post.channel_data(ch)
            data, fc, rate = chan_cache[ch]
            riq = rd.pre(data, fc, rate)
            if riq is None:
                want[i].append(None)
                continue
            words = rd.state()                       # the reference's own integer state after this block: oscillator phase word, resampler phase, half-band fill
            gpu_iq = modem_iq[i][b] if modem_iq and i in modem_iq else None
            miq = gpu_iq if gpu_iq is not None and gpu_iq.size == riq.size else riq
            out = rd.demodulate(miq)
            if cpp is not None and out is not None:
                a, ch = cpp[i].demodulate(miq)
                assert ch == out.get("channels", 1) and np.array_equal(a, out["audio"]), ("oracle glue differs from the reference's modem class", i, b)
            if out is None:       # no samples in this block: demodulate() returns at once, no audio item, no state change
                out = dict(audio=np.zeros(0, np.float32), level_accum=0.0, level_count=0, peak=0.0)
            out["iq"] = riq
            out.update(nco_theta=words["nco_theta"], resamp_phase=words["resamp_phase"], buffer_index=words["buffer_index"])
            want[i].append(out)
    for m in cpp or []:
        m.close()
    return want


_DEFAULT_BW = {"NBFM": 12500, "FM": 200000, "AM": 6000, "USB": 5400, "LSB": 5400, "I/Q": 48000, "CW": 500, "DSB": 5400}


def _run_demods(ctx, fs, M, block, kinds, n_blocks, batch, bw=None, seed=3, oversampled=False, modem_on_gpu_iq=()):
    """modem_on_gpu_iq: slots whose reference MODEM is fed the GPU's resampled IQ of each block (the reference front-end still
    runs and its IQ is compared): isolates a modem whose arithmetic amplifies the 1e-6 front-end differences."""
    center = 100000000
    freqs = demod_frequencies(center, fs, len(kinds))
    bws = [bw[k] if bw else _DEFAULT_BW[k] for k in kinds] if not isinstance(bw, list) else bw
    demods = list(zip(kinds, freqs))
    x = synth_iq(n_blocks * block, fs, center, demods, seed=seed)
    got = _gpu_demods(ctx, x, fs, M, block, demods, bws, n_blocks, batch, oversampled)
    want = _ref_demods(x, fs, M, block, demods, bws, n_blocks, oversampled,
                       modem_iq={i: [g["iq"] for g in got[i]] for i in modem_on_gpu_iq})
    return got, want


def _full_config(ctx, fs, M, block, kinds, n_blocks, seed, hist=None, persample=None):
    """every demodulator of a BASELINE configuration over n_blocks consecutive blocks: one oracle run, the HIP path once as ONE
    batch and once block at a time; both must match the oracle (counts and phase words exact, samples within TOL) and each
    other bit for bit.  Returns the worst errors."""
    center = 100000000
    freqs = demod_frequencies(center, fs, len(kinds))
    demods = list(zip(kinds, freqs))
    bws = [_DEFAULT_BW[k] for k in kinds]
    x = synth_iq_fast(n_blocks * block, fs, center, demods, seed=seed)
    want = _ref_demods(x, fs, M, block, demods, bws, n_blocks)
    # Demodulators routed to channel 0 sit behind the reference's float32 DC blocker (SDRPostThread.cpp:375), whose state
    # v ~ DC M / 0.0005 carries ~ulp(v) of rounding noise per sample that no evaluation order reproduces (the GPU evaluates the
    # recurrence to fp64 accuracy: test_dc_blocker_large_offset_state_noise).  They get that noise floor as an absolute allowance.
    dc_floor = float(4 * np.spacing(np.float32(0.01 * M / 0.0005))) if M > 1 else 0.0
    floors = {i: dc_floor for i, ch in enumerate(_ref_demods.last_channels) if ch == 0 and M >= 100}
    batched = _gpu_demods(ctx, x, fs, M, block, demods, bws, n_blocks, n_blocks)
    worst = _compare(batched, want, "batched", floors, hist, persample)
    single = _gpu_demods(ctx, x, fs, M, block, demods, bws, n_blocks, 1)
    _compare(single, want, "blockwise", floors)
    for i in range(len(kinds)):
        for a, b in zip(batched[i], single[i]):
            assert (a["n_iq"], a["n_audio"], a["nco_theta"], a["resamp_phase"], a["buffer_index"]) == (b["n_iq"], b["n_audio"], b["nco_theta"], b["resamp_phase"], b["buffer_index"]), i
            assert np.array_equal(a["audio"], b["audio"]) and np.array_equal(a["iq"], b["iq"]), i
    return dict(iq=max(w[0] for w in worst.values()), audio=max(w[1] for w in worst.values()),
                level=max(w[2] for w in worst.values()), peak=max(w[3] for w in worst.values()))


_ERR_EDGES = np.array([0.0, 1e-7, 3e-7, 1e-6, 2e-6, 4e-6, 6e-6, 8e-6, 1e-5, 1e30])


def _compare(got, want, label, floors=None, hist=None, persample=None):
    """floors: {slot: absolute noise floor of that slot's channel samples} (channel 0 behind a wide channelizer, see _full_config):
    the slot's IQ may differ by that much on top of TOL, its audio / level / peak by the phase noise that implies."""
    worst = {}
    for i in range(len(got)):
        assert len(got[i]) == len(want[i])
        ga = np.concatenate([g["audio"] for g in got[i]])
        wa = np.concatenate([w["audio"] for w in want[i]])
        gi = np.concatenate([g["iq"] for g in got[i]])
        wi = np.concatenate([w["iq"] for w in want[i]])
        for b, (g, w) in enumerate(zip(got[i], want[i])):
            assert g["n_iq"] == w["iq"].size, (label, i, b, g["n_iq"], w["iq"].size)          # bit-exact decimation index
            assert g["n_audio"] == w["audio"].size, (label, i, b, g["n_audio"], w["audio"].size)
            assert g["level_count"] == w["level_count"], (label, i, b)
            # the integer state after the block against the REFERENCE's own words (its oscillator / resampler objects, oracle/liquid_api.py:
            # nco_state, msresamp_state), not only against another run of the HIP path
            if "nco_theta" in w:
                assert (g["nco_theta"], g["resamp_phase"], g["buffer_index"]) == (w["nco_theta"], w["resamp_phase"], w["buffer_index"]), \
                    (label, i, b, (g["nco_theta"], g["resamp_phase"], g["buffer_index"]), (w["nco_theta"], w["resamp_phase"], w["buffer_index"]))
        e_iq, e_au = rel_err(gi, wi), rel_err(ga, wa)
        if hist is not None and wa.size and not (floors and i in floors):
            # EVERY audio sample's error in units of its demodulator's peak (the bound is on the maximum of these; this shows how few samples sit near it)
            hist += np.histogram(np.abs(ga - wa) / float(np.max(np.abs(wa))), bins=_ERR_EDGES)[0]
            if persample is not None:
                # ... and relative to the SAMPLE's own magnitude (not the stream's peak), floored at 1 % of the peak: a sample at a zero crossing has no scale of its own
                persample.append(np.abs(ga - wa) / np.maximum(np.abs(wa), 0.01 * float(np.max(np.abs(wa)))))
        # per-block level sums and peaks, relative to the block's own value -- but not below 5 % of the stream's peak per
        # sample (a block of one or two quiet samples has no scale of its own)
        gpk = float(np.max(np.abs(wa))) if wa.size else 1.0
        lv = max([abs(g["level_accum"] - w["level_accum"]) / max(abs(w["level_accum"]), 0.05 * gpk * max(w["level_count"], 1), 1e-30)
                  for g, w in zip(got[i], want[i]) if w["audio"].size] + [0.0])
        pk = max([abs(g["peak"] - w["peak"]) / max(abs(w["peak"]), 0.05 * gpk, 1e-30) for g, w in zip(got[i], want[i]) if w["audio"].size] + [0.0])
        worst[i] = (e_iq, e_au, lv, pk)
        tol_iq = tol_au = TOL
        if floors and i in floors and wi.size:
            tol_iq = TOL + floors[i] / float(np.max(np.abs(wi)))
            tol_au = TOL + 2.0 * floors[i] / float(np.median(np.abs(wi)))      # two noisy samples per discriminator / envelope output
            worst[i] = (0.0, 0.0, 0.0, 0.0)                                  # reported separately: not part of the configuration's worst case
            print("slot %d on channel 0: iq %.3g audio %.3g (allowances %.3g / %.3g)" % (i, e_iq, e_au, tol_iq, tol_au))
        assert e_iq < tol_iq, (label, i, "iq", e_iq)
        assert e_au < tol_au, (label, i, "audio", e_au)
        assert lv < tol_au and pk < tol_au, (label, i, lv, pk)
    return worst


def test_nbfm_c1_config(ctx):
    """BASELINE config 1 shape: 1x NBFM, 2.4 MS/s, M = 4, block 40000 (Fc = 600 kS/s), 6 consecutive blocks."""
    got, want = _run_demods(ctx, 2400000, 4, 40000, ["NBFM"], 6, 1)
    print(_compare(got, want, "c1"))


def test_nbfm_from_100k_channels_depth_two_cascade(ctx):
    """the C4 channel rate (100 MS/s / 1024 = 97 656.25 S/s) in a small frame: NBFM behind it is a TWO-stage half-band cascade (m = 5, 10) and the
    arbitrary stage at 0.512 -- the generic front-end kernel (a specialised depth-2 instance with 1024-sample chunks was measured in round 4:
    0.28 against 0.23 ms per C4 batch, not kept); AM next to it runs depth 4.  6 blocks in batches of 2."""
    got, want = _run_demods(ctx, 781250, 8, 8 * 1628, ["NBFM", "AM", "NBFM"], 6, 2, seed=23)
    print(_compare(got, want, "depth2"))


def test_mixed_modems_streaming(ctx):
    got, want = _run_demods(ctx, 2400000, 4, 40000, ["NBFM", "AM", "USB", "LSB", "NBFM", "AM", "USB"], 6, 1)
    print(_compare(got, want, "mixed"))


def test_wide_fm_audio_decimation(ctx):
    """ModemFM at its default 200 kHz (CubicSDR.cpp:305): the IQ resampler has a single half-band stage (generic front-end
    kernel) and the audio msresamp_rrrf DECIMATES (200 k -> 48 k: two half-band stages, then the arbitrary stage)."""
    got, want = _run_demods(ctx, 2400000, 4, 40000, ["FM", "NBFM", "FM"], 6, 2, seed=17)
    print(_compare(got, want, "fm"))


def test_wide_demodulators_many_samples_per_block(ctx):
    """more than 4096 resampled samples per block and demodulator (the former per-workgroup wall): FM at 400 kHz and AM at
    300 kHz on 600 kS/s channels (6667 / 5000 samples per 1/60 s block), next to an NBFM demodulator, 4 blocks in batches of 2."""
    got, want = _run_demods(ctx, 2400000, 4, 40000, ["FM", "NBFM", "AM"], 4, 2, bw=[400000, 12500, 300000], seed=19)
    assert got[0][0]["n_iq"] > 6000 and got[2][0]["n_iq"] > 4900
    print(_compare(got, want, "wide"))


def test_bandwidth_above_channel_rate_interpolating_iq_resampler(ctx):
    """demodulator bandwidths above the channel rate (msresamp_crcf with rate > 1, DemodulatorWorkerThread.cpp:97-101): FM at
    800 kHz (rate 1.33: arbitrary stage only) and 1.5 MHz (rate 2.5: arbitrary stage + one x2 half-band) on 600 kS/s channels,
    next to an NBFM demodulator; 4 blocks in batches of 2 (block boundaries inside output chunks, history across batches)."""
    got, want = _run_demods(ctx, 2400000, 4, 20000, ["FM", "NBFM", "FM"], 4, 2, bw=[800000, 12500, 1500000], seed=21)
    assert got[0][0]["n_iq"] > 6000 and got[2][0]["n_iq"] > 12000
    print(_compare(got, want, "interp"))


def _fms_case(ctx, fs, M, block, n_blocks, batch, bw=200000, seed=31, audio_rate=48000, demph=75):
    """FM stereo (ModemFMStereo.cpp) next to an NBFM demodulator.  What can and cannot be compared:
      * resampled IQ, counts, levels, the mono path and the SUM of the output channels (l + r = 2 x 0.568 x filtered mono: the
        stereo-difference stream cancels) -- within TOL like every other modem;
      * the pilot loop limit-cycles on the oscillator table's 2 pi / 1024 phase steps (bandwidth 0.25 loop), so the reference's own
        l - r moves by ~1e-3 of the peak when its input IQ moves by a tenth of the 1e-5 parity tolerance: the HIP path's l - r must be
        as close to the reference's as the reference is to itself under that perturbation (measured here, same signal);
      * given the HIP path's own oscillator phases, its down-mix + c2r Hilbert stage is pinned against the reference's functions at TOL.
    Returns the measured figures."""
    import ctypes as C
    import oracle.liquid_api as A
    from oracle.cubicsdr_chain import RefDemod, RefSDRPost
    from cubicsdr_amd.engine import DemodBank, SDRPost
    if not A.available("ref"):
        pytest.skip("the FM stereo oracle needs the reference liquid binary (oracle/_ref)")
    L = A.load("ref")
    center = 100000000
    kinds = ["FMS", "NBFM"]
    freqs = demod_frequencies(center, fs, 2)
    demods = list(zip(kinds, freqs))
    x = synth_iq(n_blocks * block, fs, center, demods, seed=seed)
    L.ref_peek.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    L.ref_poke.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    # ---- reference, twice: the second modem is fed the same resampled IQ plus noise of a TENTH of the IQ stream's parity tolerance
    prng = np.random.default_rng(seed + 1)
    ref_post = RefSDRPost("ref", fs, M)
    r0 = RefDemod("ref", "FMS", bw, freqs[0], ref_post.chan_bw, audio_rate=audio_rate, demph=demph)
    r1 = RefDemod("ref", "FMS", bw, freqs[0], ref_post.chan_bw, audio_rate=audio_rate, demph=demph)
    want, pert = [], []
    for b in range(n_blocks):
        ref_post.run_block(x[b * block:(b + 1) * block], center)
        data, fc, rate = ref_post.channel_data(ref_post.channel_at(freqs[0]))
        riq = r0.pre(data, fc, rate)
        out = r0.demodulate(riq)
        out["iq"] = riq
        want.append(out)
        # (relative noise: the resampler's first outputs are ~0 and their phase -- the discriminator's input -- has no scale)
        noise = (prng.standard_normal(riq.size) + 1j * prng.standard_normal(riq.size)) * (0.1 * TOL)
        pert.append(r1.demodulate((riq * (1.0 + noise)).astype(np.complex64)))
    # ---- HIP path
    post = SDRPost(ctx, fs, M, block, max_blocks=batch)
    bank = DemodBank(ctx, 2, max_blocks=batch)
    bank.configure(0, post, "FMS", bw, freqs[0], audio_sample_rate=audio_rate, modem_arg=demph if demph else -1)
    bank.configure(1, post, "NBFM", 12500, freqs[1])
    got, theta, sdiff = [], [], []
    for b0 in range(0, n_blocks, batch):
        post.execute(x[b0 * block:(b0 + batch) * block], batch, block, center)
        bank.execute(post)
        res, audio, iq = bank.results(0), bank.audio(0), bank.iq(0)
        theta.append(bank.fms_stage(0, 0)); sdiff.append(bank.fms_stage(0, 1))
        o = 0
        for r in res:
            got.append(dict(n_iq=r.n_iq, n_audio=r.n_audio, audio=audio[r.audio_offset:r.audio_offset + r.n_audio], iq=iq[o:o + r.n_iq],
                            level_accum=r.level_accum, level_count=r.level_count, peak=r.audio_peak))
            o += r.n_iq
    assert bank.demod_output(0).size == 0                       # not a ModemAnalog: no demodOutputData tap
    post.close(); bank.close()
    theta = np.concatenate(theta); sdiff = np.concatenate(sdiff)
    if batch > 1:
        # block at a time: the pilot filter / loop state, the Hilbert windows, both resamplers and the output filters carry across
        # every block boundary exactly as they do inside a batch -- same bits
        post = SDRPost(ctx, fs, M, block, max_blocks=1)
        bank = DemodBank(ctx, 2, max_blocks=1)
        bank.configure(0, post, "FMS", bw, freqs[0], audio_sample_rate=audio_rate, modem_arg=demph if demph else -1)
        bank.configure(1, post, "NBFM", 12500, freqs[1])
        th1 = []
        for b in range(n_blocks):
            post.execute(x[b * block:(b + 1) * block], 1, block, center)
            bank.execute(post)
            r = bank.results(0)[0]
            assert (r.n_iq, r.n_audio) == (got[b]["n_iq"], got[b]["n_audio"]), b
            assert np.array_equal(bank.audio(0)[:r.n_audio], got[b]["audio"]), b
            th1.append(bank.fms_stage(0, 0))
        assert np.array_equal(np.concatenate(th1), theta)
        post.close(); bank.close()
    # ---- counts, IQ, levels
    for b, (g, w) in enumerate(zip(got, want)):
        assert g["n_iq"] == w["iq"].size and g["n_audio"] == w["audio"].size and g["level_count"] == w["level_count"], b
        assert abs(g["level_accum"] - w["level_accum"]) <= 1e-5 * abs(w["level_accum"]), b
    gi, wi = np.concatenate([g["iq"] for g in got]), np.concatenate([w["iq"] for w in want])
    ga, wa, pa = (np.concatenate([q["audio"] for q in lst]) for lst in (got, want, pert))
    peak = float(np.max(np.abs(wa)))
    e_iq = rel_err(gi, wi)
    assert e_iq < TOL, e_iq
    # ---- sum and difference of the output channels
    e_sum = float(np.max(np.abs((ga[0::2] + ga[1::2]) - (wa[0::2] + wa[1::2])))) / peak
    e_diff = float(np.max(np.abs((ga[0::2] - ga[1::2]) - (wa[0::2] - wa[1::2])))) / peak
    self_diff = float(np.max(np.abs((pa[0::2] - pa[1::2]) - (wa[0::2] - wa[1::2])))) / peak
    self_sum = float(np.max(np.abs((pa[0::2] + pa[1::2]) - (wa[0::2] + wa[1::2])))) / peak
    assert e_sum < TOL, e_sum
    assert self_sum < TOL                                        # (the perturbation itself is invisible in the mono path)
    assert self_diff > 10 * TOL, self_diff                       # the reference is THIS sensitive: the premise of the looser bound below
    assert e_diff < 4 * self_diff, (e_diff, self_diff)
    # the difference channel must still BE the stereo difference: its 700 Hz / 1 kHz content correlates with the reference's
    gd, wd = ga[0::2] - ga[1::2], wa[0::2] - wa[1::2]
    k0 = gd.size // 3
    corr = float(np.dot(gd[k0:], wd[k0:]) / np.sqrt(np.dot(gd[k0:], gd[k0:]) * np.dot(wd[k0:], wd[k0:])))
    assert corr > 0.9999, corr
    assert float(np.sqrt(np.mean(wd[k0:] ** 2))) > 0.05 * peak   # (and it is not silence)
    # ---- pilot loop: locked on 19 kHz, and within a few table steps of the reference's phase
    wt = np.concatenate([w["fms_theta"] for w in want])
    n0 = theta.size // 3
    turns = np.cumsum(((np.diff(theta[n0:].astype(np.int64)) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.float64)) / 2 ** 32
    f_lock = turns[-1] / (theta.size - n0 - 1) * max(bw, 100000)
    assert want[0]["iq"].size * (fs / block) > 0.9 * max(bw, 100000)       # (the modem really runs at checkSampleRate(bw))
    wturns = np.cumsum(((np.diff(wt[n0:].astype(np.int64)) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.float64)) / 2 ** 32
    f_ref = wturns[-1] / (wt.size - n0 - 1) * max(bw, 100000)
    assert abs(f_lock - f_ref) < 2.0, (f_lock, f_ref)           # the same lock as the reference's loop ...
    if bw >= 150000:
        assert abs(f_lock - 19000.0) < 2.0, f_lock               # ... which is the pilot when the multiplex fits the modem bandwidth
    dth = ((theta.astype(np.int64) - wt.astype(np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31) * (2 * np.pi / 2 ** 32)
    assert float(np.sqrt(np.mean(dth[n0:] ** 2))) < 4 * 2 * np.pi / 1024, float(np.sqrt(np.mean(dth[n0:] ** 2)))
    # ---- down-mix + c2r stage, given the HIP path's own phases: the reference's r2c / table oscillator / c2r functions on the
    # reference's discriminator output (equal to the HIP path's within TOL) with the oscillator's phase word set per sample
    d = np.concatenate([w["demod"] for w in want])
    r2c, c2r, osc = L.firhilbf_create(5, 60.0), L.firhilbf_create(5, 60.0), L.nco_crcf_create(A.LIQUID_VCO)
    xs, y1, y2 = A.cf32(), A.cf32(), A.cf32()
    lo, up = C.c_float(), C.c_float()
    nchk = min(d.size, 30000)
    s_ref = np.empty(nchk, np.float32)
    word = np.zeros(1, np.uint32)
    for i in range(nchk):
        L.firhilbf_r2c_execute(C.c_void_p(r2c), float(d[i]), C.byref(xs))
        word[0] = theta[i]
        L.ref_poke(C.c_void_p(osc), 0x1004, A.ptr(word), 4)
        L.nco_crcf_mix_down(C.c_void_p(osc), xs, C.byref(y1))
        L.nco_crcf_mix_down(C.c_void_p(osc), y1, C.byref(y2))
        L.firhilbf_c2r_execute(C.c_void_p(c2r), y2, C.byref(lo), C.byref(up))
        s_ref[i] = lo.value
    e_mix = rel_err(sdiff[:nchk], s_ref)
    assert e_mix < TOL, e_mix
    return dict(iq=e_iq, sum=e_sum, diff=e_diff, ref_self_diff=self_diff, mix_stage=e_mix, lock_hz=float(f_lock), corr=corr,
                theta_rms=float(np.sqrt(np.mean(dth[n0:] ** 2))))


@pytest.mark.parametrize("bw,audio_rate,demph", [(250000, 44100, 50), (150000, 48000, 0), (50000, 48000, 75),
                                                 (100000, 192000, 75), (100000, 120000, 50)])     # the last two: audio ABOVE the modem rate (interpolating audio resamplers, ModemFMStereo.cpp:91-105)
def test_fm_stereo_settings(ctx, bw, audio_rate, demph):
    """other modem rates (250 kHz; 150 kHz; 50 kHz -> checkSampleRate lifts it to 100 kHz), 44.1 kHz audio, 50 us and no de-emphasis"""
    print("fms", bw, audio_rate, demph, _fms_case(ctx, 2400000, 4, 40000, 4, 2, bw=bw, audio_rate=audio_rate, demph=demph, seed=37))


def test_fm_stereo_modem(ctx):
    """ModemFMStereo at its default 200 kHz on a 600 kS/s channel (audio resamplers decimate 200 kHz -> 48 kHz), 6 blocks of 1/60 s
    in batches of 3: state carried across blocks and batches (pilot filter, loop, Hilbert windows, both resamplers, output filters)."""
    print("fms", _fms_case(ctx, 2400000, 4, 40000, 6, 3))


def test_batched_equals_reference(ctx):
    """6 blocks in two batches of 3: results must equal the block-at-a-time reference (counts exact)."""
    got, want = _run_demods(ctx, 2400000, 4, 40000, ["NBFM", "AM", "USB"], 6, 3)
    print(_compare(got, want, "batched"))


def test_c2_shape_64_nbfm(ctx):
    """BASELINE config 2 (64x NBFM, 10 MS/s, M = 20, block 166 680): ALL 64 demodulators over 3 consecutive blocks against the
    oracle, as one 3-block batch and block at a time."""
    print("c2 worst errors", _full_config(ctx, 10000000, 20, 166680, ["NBFM"] * 64, 3, seed=23))


def test_iq_passthrough_modem(ctx):
    """ModemIQ: the bandwidth is forced to the audio rate, the "audio" is the resampled IQ as stereo frames (imag, real);
    next to an NBFM demodulator on the same channelizer, 6 blocks in batches of 3."""
    got, want = _run_demods(ctx, 2400000, 4, 40000, ["I/Q", "NBFM", "I/Q"], 6, 3, seed=29)
    print(_compare(got, want, "iq"))
    assert got[0][0]["n_audio"] == 2 * got[0][0]["n_iq"]


def test_cw_modem(ctx):
    """ModemCW: 500 Hz of IQ interpolated x96 to the audio rate (msresamp_cccf: arbitrary stage + six x2 stages), 650 Hz beep
    oscillator, c2r Hilbert, auto-gain through dB.  14 blocks so that the keyed carrier is well through the 500 S/s filters;
    batches of 7 exercise the gain replay and the oscillator / resampler phases across batches."""
    # (a 32 kS/s channel: from the 600 kS/s channels of the other tests 500 Hz would take a ten-stage IQ cascade, which the
    #  front-end does not carry history for)
    got, want = _run_demods(ctx, 128000, 4, 2132, ["CW", "NBFM", "CW"], 14, 7, seed=33)
    w = _compare(got, want, "cw")
    print(w)
    assert max(g["peak"] for g in got[0]) > 0.05          # the tone actually came through


def test_dsb_modem_costas_loop(ctx):
    """ModemDSB: liquid's suppressed-carrier DSB demodulator is a Costas loop (per-sample phase feedback into the table
    oscillator, phase-word quantised), so one thread walks each demodulator's batch; the carrier is 35 Hz off tune and the
    loop has to pull in.  8 blocks in batches of 1, 3 and 4: the loop state crosses batch boundaries."""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    # The loop's hard decision (sign of Re v) flips on a 1e-6 input difference whenever Re v passes through zero, and a flipped
    # step perturbs the phase for many samples (observed 4e-4 for a few blocks): no implementation can track the reference
    # through that from inputs that differ in the last bits.  So the reference MODEM is run on the GPU's own resampled IQ
    # (which is separately held to 1e-5 of the reference's) and the demodulator has to reproduce it sample for sample.
    got, want = _run_demods(ctx, 2400000, 4, 40000, ["DSB", "NBFM", "DSB"], 8, 4, seed=37, modem_on_gpu_iq=(0, 2))
    print(_compare(got, want, "dsb"))
    got1, want1 = _run_demods(ctx, 2400000, 4, 40000, ["DSB"], 3, 1, seed=38, modem_on_gpu_iq=(0,))
    print(_compare(got1, want1, "dsb1"))
    # end to end against the reference front-end the audio still agrees to a fraction of a percent
    got2, want2 = _run_demods(ctx, 2400000, 4, 40000, ["DSB"], 8, 4, seed=37)
    ga = np.concatenate([g["audio"] for g in got2[0]]); wa = np.concatenate([w["audio"] for w in want2[0]])
    assert rel_err(ga, wa) < 5e-3


def test_cw_from_a_wide_channel_ten_stage_cascade(ctx):
    """500 Hz CW straight from a 600 kS/s channel: the IQ msresamp_crcf runs TEN half-band stages (span ~46 000 inputs, more
    than a block: the carried mixed-input history and the warm-up re-derivation are exercised at their deepest)."""
    got, want = _run_demods(ctx, 2400000, 4, 40000, ["CW", "NBFM"], 12, 4, seed=35)
    print(_compare(got, want, "cw10"))


def test_demods_behind_oversampled_channelizer(ctx):
    """chanMode 2: the demodulators see their channel at 2 * chanBw (runDemodChannels(chanBw * 2), :510), so the IQ
    resampler ratio and cascade depth change; mixed modems over 6 blocks in batches of 2."""
    got, want = _run_demods(ctx, 2400000, 4, 40000, ["NBFM", "AM", "USB", "FM", "LSB"], 6, 2, seed=23, oversampled=True)
    print(_compare(got, want, "pfbch2"))


def test_tiny_blocks_ragged_outputs(ctx):
    """Blocks far shorter than the filters: 400 input samples = 100 channel samples -> two or three resampled IQ samples and
    a handful of audio samples per block, some blocks of the narrow modems produce none at all.  Every cascade reaches
    back over many blocks (the auto-gain of the block a history sample belongs to is replayed), counts stay exact."""
    got, want = _run_demods(ctx, 2400000, 4, 400, ["NBFM", "AM", "USB", "I/Q"], 60, 15, seed=43)
    print(_compare(got, want, "tiny"))
    assert min(g["n_audio"] for g in got[1]) <= 1 or min(g["n_iq"] for g in got[1]) <= 1


def test_single_channel_mode_demod(ctx):
    got, want = _run_demods(ctx, 480000, 1, 8000, ["NBFM", "AM"], 5, 1)
    print(_compare(got, want, "single"))


# ----------------------------------------------------------------------------------------------- spectrum
@pytest.mark.parametrize("F", [512, 2048, 16384, 65536, 600, 1000, 750, 37, 3, 1023, 1025, 1500, 3000, 5000, 12345, 50000, 100001])
def test_fft_matches_liquid(ctx, F):
    """fft_execute (SpectrumVisualProcessor.cpp:439) at the sizes the GUI sets and -- setFFTSize takes any size (:180-190) -- at sizes that are
    not powers of two (chirp-z transform; internal 2 x fftSize points, odd fftSize included; above fftSize 1024 the convolution runs as two
    power-of-two transform chains of 8192 .. 2^19 points in HBM)"""
    from cubicsdr_amd.engine import SpectrumProcessor
    from oracle.cubicsdr_chain import RefSpectrum
    x = synth_iq(2 * F, 2.4e6, 0, [("NBFM", 300000.0)], seed=77)
    sp = SpectrumProcessor(ctx, F, max_frames=1)
    ref = RefSpectrum(_backend(), F)
    assert rel_err(sp.fft_only(x), ref.fft(x)) < TOL
    sp.close()


@pytest.mark.parametrize("F,block", [(2048, 40000), (16384, 166680), (600, 40000), (375, 4000), (65536, 1024068)])
def test_spectrum_points_first_frame_mode(ctx, F, block):
    from cubicsdr_amd.engine import SpectrumProcessor
    from oracle.cubicsdr_chain import RefSpectrum
    fs = 10000000 if F == 16384 else 2400000
    nb = 5
    x = synth_iq(nb * block, fs, 0, [("NBFM", 300000.0), ("AM", -500000.0)], seed=9)
    sp = SpectrumProcessor(ctx, F, max_frames=nb)
    ref = RefSpectrum(_backend(), F)
    # 3 blocks one at a time, then 2 in one call
    for b in range(3):
        assert sp.process(x[b * block:(b + 1) * block], 1, block) == 1
        pts, ce, fl = sp.fetch(0)
        wp, wce, wfl = ref.process_frame(x[b * block:b * block + 2 * F])
        assert rel_err(pts, wp) < TOL, b
        assert abs(ce - wce) <= TOL * abs(wce) and abs(fl - wfl) <= TOL * abs(wce), b
    assert sp.process(x[3 * block:5 * block], 2, block) == 2
    for k in range(2):
        pts, ce, fl = sp.fetch(k)
        wp, wce, wfl = ref.process_frame(x[(3 + k) * block:(3 + k) * block + 2 * F])
        assert rel_err(pts, wp) < TOL, k
        assert abs(ce - wce) <= TOL * abs(wce), k
    sp.close()


def test_spectrum_contiguous_mode(ctx):
    from cubicsdr_amd.engine import SpectrumProcessor
    from oracle.cubicsdr_chain import RefSpectrum
    F, block, nb = 2048, 10000, 4
    x = synth_iq(nb * block, 2.4e6, 0, [("NBFM", 300000.0)], seed=10)
    sp = SpectrumProcessor(ctx, F, max_frames=8)
    ref = RefSpectrum(_backend(), F)
    done = 0
    for b in range(nb):
        nf = sp.process(x[b * block:(b + 1) * block], 1, block, contiguous=True)
        for k in range(nf):
            pts, ce, fl = sp.fetch(k)
            wp, wce, wfl = ref.process_frame(x[done * 2 * F:(done + 1) * 2 * F])
            assert rel_err(pts, wp) < TOL, (b, k)
            done += 1
    assert done == (nb * block) // (2 * F)
    sp.close()


@pytest.mark.parametrize("F,line", [(2048, 2048), (2048, 3000), (1024, 600), (16384, 16384), (65536, 65536), (65536, 100000)])
def test_spectrum_line_cadence_overlapped_frames(ctx, F, line):
    """FFTDataDistributor hands the spectrum fftSize-sample lines (FFTDataDistributor.cpp:112-131), shorter than the
    2*fftSize transform: the first primes fftLastData, every later one is transformed together with the tail of the
    previous FFT input (SpectrumVisualProcessor.cpp:399-421).  Lines one at a time, then several per call."""
    from cubicsdr_amd.engine import SpectrumProcessor
    from oracle.cubicsdr_chain import RefSpectrum
    nl = 11
    x = synth_iq(nl * line, 2.4e6, 0, [("NBFM", 300000.0), ("AM", -400000.0)], seed=21)
    sp = SpectrumProcessor(ctx, F, max_frames=8)
    ref = RefSpectrum(_backend(), F)
    want = []
    exact = None
    if F >= 65536:
        exact = exact_spectrum(_backend(), F)             # the same restatement with a float64 transform
    exact_all = []
    for k in range(nl):
        fr = ref.select_input(x[k * line:(k + 1) * line])
        want.append(None if fr is None else ref.process_frame(fr))
        exact_all.append(None if (fr is None or exact is None) else exact.process_frame(np.array(fr)))
    assert want[0] is None and all(w is not None for w in want[1:])
    worst_seen = [0.0, 0.0, 0.0]
    k = 0
    for per_call in (1, 1, 1, 3, 5):
        nf = sp.process(x[k * line:(k + per_call) * line], per_call, line, lines=True)
        expect = [w for w in want[k:k + per_call] if w is not None]
        exact_frames = {k + j: ew for j, ew in enumerate([q for q, w in zip(exact_all[k:k + per_call], want[k:k + per_call]) if w is not None])}
        assert nf == len(expect), (k, nf)
        for j, (wp, wce, wfl) in enumerate(expect):
            pts, ce, fl = sp.fetch(j)
            e = rel_err(pts, wp)
            if exact is None:
                assert e < TOL, (k, j)
            else:
                # 2^17-point frames of a SPARSE signal (two strong carriers over a noise floor: the float32 transform's rounding noise in the weak
                # bins is set by the carriers) in the first inputs after the start, while the floor tracker is still ~ 5e-5: one point of 65536
                # can sit 1e-5 of display value from the reference's own float32 result, on either side of the exact value
                # (profiles/experiments/r05_lines_err.py: the reference is 5.2e-6 from a float64 transform of the same frame, the two HIP chains
                # 5.5e-6 / 8.4e-6, with the same error distribution otherwise: rms 1.5e-7).  Held as the 2^21-point frames are (DESIGN 2,
                # deviation 5): no further from the exact result than the tolerance or 1.5 x the reference's distance, and within the tolerance
                # + both distances of the reference.
                ew = exact_frames[k + j]
                e_ref, e_hip = rel_err(wp, ew[0]), rel_err(pts, ew[0])
                worst_seen[0] = max(worst_seen[0], e); worst_seen[1] = max(worst_seen[1], e_hip); worst_seen[2] = max(worst_seen[2], e_ref)
                assert e_hip < max(TOL, 1.5 * e_ref), (k, j, e_hip, e_ref)
                assert e < TOL + e_ref + e_hip, (k, j, e, e_ref, e_hip)
            assert abs(ce - wce) <= TOL * abs(wce) and abs(fl - wfl) <= TOL * abs(wce), (k, j)
        k += per_call
    assert k == nl
    if exact is not None:
        print("lines F=%d line=%d: worst |hip - ref| %.3g, |hip - exact| %.3g, |ref - exact| %.3g" % (F, line, *worst_seen))
    sp.close()


def test_spectrum_peak_hold_and_hide_dc(ctx):
    """setPeakHold: one input later the held arrays are reset to the floor tracker, from then on every frame carries
    spectrum_hold_points and is scaled by the held ceiling / floor; enabling again restarts a 30-input countdown.  The
    reset falls inside a batch, at its first frame, and between batches.  setHideDC rewrites the bins around the
    input's centre frequency."""
    from cubicsdr_amd.engine import SpectrumProcessor
    from oracle.cubicsdr_chain import RefSpectrum
    F, block, fs = 2048, 6000, 2400000
    nb = 60
    x = synth_iq(nb * block, fs, 0, [("NBFM", 300000.0), ("AM", -500000.0)], seed=31)
    amp = np.repeat(1.0 + 0.8 * np.sin(np.arange(nb) * 0.7), block).astype(np.float32)      # peaks must actually be held
    x = (x * amp).astype(np.complex64)
    sp = SpectrumProcessor(ctx, F, max_frames=16)
    ref = RefSpectrum(_backend(), F)
    sp.set_hide_dc(True, center_freq=100000000, bandwidth=fs, input_freq=100000000)
    ref.set_hide_dc(True, 100000000, fs, 100000000)
    plan = [(3, None), (4, True), (1, None), (6, None), (5, True), (16, None), (14, None), (6, False), (5, None)]
    k = 0
    held = 0
    for per_call, toggle in plan:
        if toggle is not None:
            sp.set_peak_hold(toggle)
            ref.set_peak_hold(toggle)
        assert sp.process(x[k * block:(k + per_call) * block], per_call, block) == per_call
        for j in range(per_call):
            wp, wce, wfl, whold = ref.process_input(x[(k + j) * block:(k + j + 1) * block])
            pts, ce, fl = sp.fetch(j)
            hold = sp.fetch_hold(j)
            assert rel_err(pts, wp) < TOL, (k, j)
            assert abs(ce - wce) <= TOL * abs(wce) and abs(fl - wfl) <= TOL * abs(wce), (k, j)
            assert (hold is None) == (whold is None), (k, j)
            if hold is not None:
                assert rel_err(hold, whold) < TOL, (k, j)
                held += 1
        k += per_call
    assert k == nb and held >= 12
    sp.close()


def test_spectrum_zoomed_view(ctx, F=512):
    """setView: the input is shifted to the view centre and resampled to the smallest rate/2^k that still covers the view
    bandwidth, then transformed; the display walks bandwidth / resampleBw bins per point.  The scenario retunes the view
    (the averagers shift), zooms in and out (they are stretched / squeezed, the resampler is rebuilt while the NCO phase
    lives on), centres the view on the input (no mixing), holds peaks across a reset, and feeds inputs shorter than the
    resampler needs (overlap rule)."""
    from cubicsdr_amd.engine import SpectrumProcessor
    from oracle.cubicsdr_chain import RefSpectrum
    fs, center = 2400000, 100000000
    block = 40000
    steps = [  # (view centre, view bandwidth, samples of the block handed over, peak-hold toggle)
        (center + 200000, 500000, block, None), (center + 200000, 500000, block, None), (center + 200000, 500000, block, True),
        (center + 200000, 500000, block, None), (center + 230000, 500000, block, None), (center + 230000, 500000, block, None),
        (center + 150000, 500000, block, None), (center + 150000, 250000, block, None), (center + 150000, 250000, block, None),
        (center + 150000, 250000, 7000, None), (center + 150000, 250000, 7000, None), (center + 150000, 250000, block, None),
        (center + 150000, 900000, block, None), (center + 150000, 900000, block, None), (center, 900000, block, None),
        (center, 900000, block, None), (center - 300000, 140000, block, None), (center - 300000, 140000, block, None),
    ]
    steps += [(center - 300000, 140000, block, None)] * 34          # long enough for the 30-input peak countdown to end
    x = synth_iq(len(steps) * block, fs, center, [("NBFM", center + 200000.0), ("AM", center + 100000.0), ("NBFM", center - 310000.0)], seed=51)
    sp = SpectrumProcessor(ctx, F, max_frames=1)
    ref = RefSpectrum(_backend(), F)
    ref.set_hide_dc(True, 0, 0, 0)
    sp.set_hide_dc(True)
    frames = held = 0
    for k, (vc, vbw, n, toggle) in enumerate(steps):
        if toggle is not None:
            sp.set_peak_hold(toggle)
            ref.set_peak_hold(toggle)
        sp.set_view(True, vc, vbw)
        ref.set_view(True, vc, vbw)
        xin = x[k * block:k * block + n]
        want = ref.process_input(xin, center, fs)
        nf = sp.process_view_input(xin, center, fs)
        assert sp.desired_input_size == ref.desired_input_size, k
        assert nf == (0 if want is None else 1), k
        if want is None:
            continue
        wp, wce, wfl, whold = want
        pts, ce, fl = sp.fetch(0)
        hold = sp.fetch_hold(0)
        assert rel_err(pts, wp) < TOL, (k, rel_err(pts, wp))
        assert abs(ce - wce) <= TOL * abs(wce) and abs(fl - wfl) <= TOL * abs(wce), k
        assert (hold is None) == (whold is None), k
        if hold is not None:
            assert rel_err(hold, whold) < TOL, k
            held += 1
        frames += 1
    assert frames >= len(steps) - 3 and held >= 3, (frames, held)
    sp.close()


@pytest.mark.parametrize("F", [600, 1500])
def test_spectrum_zoomed_view_at_sizes_that_are_not_powers_of_two(ctx, F):
    """the same walk (retunes, zoom steps, short inputs, peak hold) at fftSize 600 (chirp-z in LDS) and 1500 (the convolution as two 8192-point chains).
    (An odd fftSize is not walked: with 2 fftSize not a multiple of four the reference's zoom-out reads fft_result_ma one element past its end,
    SpectrumVisualProcessor.cpp:471 -- the HIP path puts a zero there.)"""
    test_spectrum_zoomed_view(ctx, F)


def test_spectrum_zoomed_view_behind_a_two_pass_transform(ctx):
    """the zoomed view at fftSize 4096 (8192-point transform = a radix-2 column pass + 4096-point rows): behind a multi-pass transform the
    averagers live in PAIR order (spec_state_index), so a retune (shift), a zoom step in and one out have to move them through that order
    (SpectrumVisualProcessor.cpp:316-331, :454-492); peak hold across the steps."""
    from cubicsdr_amd.engine import SpectrumProcessor
    from oracle.cubicsdr_chain import RefSpectrum
    F, fs, center = 4096, 2400000, 100000000
    block = 40000
    steps = [  # (view centre, view bandwidth, peak-hold toggle)
        (center + 200000, 500000, None), (center + 200000, 500000, None), (center + 200000, 500000, True), (center + 200000, 500000, None),
        (center + 230000, 500000, None), (center + 230000, 500000, None),              # retune: the averagers shift
        (center + 230000, 1000000, None), (center + 230000, 1000000, None),            # zoom out
        (center + 170000, 500000, None), (center + 170000, 500000, None),              # zoom in and shift
        (center, 1000000, None), (center, 1000000, None)]                              # centred on the input: no mixing
    x = synth_iq(len(steps) * block, fs, center, [("NBFM", center + 200000.0), ("AM", center + 100000.0), ("NBFM", center - 310000.0)], seed=53)
    sp = SpectrumProcessor(ctx, F, max_frames=1)
    ref = RefSpectrum(_backend(), F)
    ref.set_hide_dc(True, 0, 0, 0)
    sp.set_hide_dc(True)
    frames = held = 0
    for k, (vc, vbw, toggle) in enumerate(steps):
        if toggle is not None:
            sp.set_peak_hold(toggle)
            ref.set_peak_hold(toggle)
        sp.set_view(True, vc, vbw)
        ref.set_view(True, vc, vbw)
        xin = x[k * block:(k + 1) * block]
        want = ref.process_input(xin, center, fs)
        nf = sp.process_view_input(xin, center, fs)
        assert sp.desired_input_size == ref.desired_input_size, k
        assert nf == (0 if want is None else 1), k
        if want is None:
            continue
        wp, wce, wfl, whold = want
        pts, ce, fl = sp.fetch(0)
        hold = sp.fetch_hold(0)
        assert rel_err(pts, wp) < TOL, (k, rel_err(pts, wp))
        assert abs(ce - wce) <= TOL * abs(wce) and abs(fl - wfl) <= TOL * abs(wce), k
        assert (hold is None) == (whold is None), k
        if hold is not None:
            assert rel_err(hold, whold) < TOL, k
            held += 1
        frames += 1
    assert frames >= len(steps) - 2 and held >= 1, (frames, held)      # (a view change restarts the peak countdown: few held frames in twelve steps)
    sp.close()


def test_spectrum_many_frames_one_batch(ctx):
    """300 frames in ONE process() call (the averaging kernel splits a batch into 16 frame groups per round of 256
    frames and chains rounds): every frame must equal the frame-at-a-time reference."""
    from cubicsdr_amd.engine import SpectrumProcessor
    from oracle.cubicsdr_chain import RefSpectrum
    F, nfr = 512, 300
    N = 2 * F
    x = synth_iq(nfr * N, 2.4e6, 0, [("NBFM", 300000.0), ("AM", -400000.0)], seed=12)
    sp = SpectrumProcessor(ctx, F, max_frames=nfr)
    ref = RefSpectrum(_backend(), F)
    assert sp.process(x, 1, nfr * N, contiguous=True) == nfr
    for k in range(nfr):
        wp, wce, wfl = ref.process_frame(x[k * N:(k + 1) * N])
        if k in (0, 1, 15, 16, 17, 18, 19, 37, 255, 256, 257, 271, 272, 298, 299):
            pts, ce, fl = sp.fetch(k)
            assert rel_err(pts, wp) < TOL, k
            assert abs(ce - wce) <= TOL * abs(wce) and abs(fl - wfl) <= TOL * abs(wce), k
    # a second batch continues from the carried averager / tracker state
    y = synth_iq(20 * N, 2.4e6, 0, [("NBFM", 300000.0)], seed=13)
    assert sp.process(y, 1, 20 * N, contiguous=True) == 20
    for k in range(20):
        wp, wce, wfl = ref.process_frame(y[k * N:(k + 1) * N])
    pts, ce, fl = sp.fetch(19)
    assert rel_err(pts, wp) < TOL
    assert abs(ce - wce) <= TOL * abs(wce)
    sp.close()


def _ref_spectrum_frames(F, fs):
    """per-frame checker for the large spectrum shapes: the reference's OWN SpectrumVisualProcessor (oracle/_ref/libref_spectrum.so,
    compiled unmodified) where it travelled, else the pinned Python restatement.  Returns f(frame) -> (points, ceiling, floor)."""
    import oracle.ref_modems as RM
    from oracle.cubicsdr_chain import RefSpectrum
    if _backend() == "ref" and RM.spectrum_available():
        cpp = RM.RefSpectrumCpp(F, fs)
        cpp.set_center(0); cpp.set_bandwidth(fs)                       # full span: bandwidth == the input rate (visualRatio 1, :534)

        def step(frame):
            pts, ce, fl, _ = cpp.process(frame, 0, fs)
            return pts, ce, fl
        return step, "reference class"
    ref = RefSpectrum(_backend(), F)
    return ref.process_frame, "restatement"


@pytest.mark.parametrize("F,fs,frames_per_batch", [(65536, 61440000, (320, 300, 333)), (16384, 10000000, (300, 520, 301))])
def test_spectrum_headline_shape_contiguous_batches(ctx, F, fs, frames_per_batch):
    _spectrum_contiguous_batches(ctx, F, fs, frames_per_batch)


def test_spectrum_chain_switch_on_five_streams_without_host_waits():
    """the fused chain's intermediate rows are read by its row pass on the averaging lane: with CSDR_STREAMS=5 (transform and averaging on streams of
    their own) a batch of the three-kernel chain that follows a fused one -- peak hold switched on between two calls, nothing fetched in between --
    must not start rewriting them early.  Back-to-back calls on five streams give the frames the one-stream context gives, bit for bit."""
    import os
    from cubicsdr_amd.engine import Context, SpectrumProcessor
    F, fs, block, nb = 65536, 61440000, 1024068, 6
    x = synth_iq(nb * block, fs, 100000000, [("NBFM", 100000000 + 1234567), ("AM", 100000000 - 20000000)], seed=78)
    outs = []
    for streams in ("1", "5"):
        old = os.environ.get("CSDR_STREAMS")
        os.environ["CSDR_STREAMS"] = streams
        try:
            c = Context(0)
        finally:
            if old is None:
                os.environ.pop("CSDR_STREAMS", None)
            else:
                os.environ["CSDR_STREAMS"] = old
        sp = SpectrumProcessor(c, F, max_frames=10)
        res = []
        for rep in range(3):                                   # the hazard is a timing one: a few rounds of fused, fused, held, held, fused, fused
            for b in range(nb):
                if b == 2:
                    sp.set_peak_hold(True)
                if b == 4:
                    sp.set_peak_hold(False)
                n = sp.process(x[b * block:(b + 1) * block], 1, block, contiguous=True)
                if b in (3, 5):
                    res.append(np.concatenate([sp.fetch(i)[0] for i in range(n)]))
        sp.close(); c.close()
        outs.append(res)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_spectrum_headline_small_calls_and_chain_switch(ctx):
    """the fused two-pass chain of the headline size (N = 2^17) in the real-time shape: ONE 1/60 s block per call (7 or 8 frames: partial
    rounds of the row pass, one frame group per column workgroup, a partial frame carried from call to call) produces exactly the frames ONE
    batch over the same samples does; and peak hold switched on and off in the stream (since round 6 inside the fused chain: the row pass keeps the held
    maxima, the reset falls inside a call): every frame and every held line against the reference's class."""
    from cubicsdr_amd.engine import SpectrumProcessor
    F, fs, block = 65536, 61440000, 1024068
    nb = 5
    x = synth_iq(nb * block, fs, 100000000, [("NBFM", 100000000 + 1234567), ("AM", 100000000 - 20000000)], seed=77)
    one = SpectrumProcessor(ctx, F, max_frames=(nb * block) // (2 * F) + 2)
    nf = one.process(x, nb, block, contiguous=True)
    want = [one.fetch(k) for k in range(nf)]
    calls = SpectrumProcessor(ctx, F, max_frames=10)
    got = []
    for b in range(nb):
        n = calls.process(x[b * block:(b + 1) * block], 1, block, contiguous=True)
        assert n in (7, 8)
        got += [calls.fetch(k) for k in range(n)]
    assert len(got) == nf
    for k in range(nf):
        # (the trackers of a batch are weighted sums over its frames, closed form in double: another batching is another summation order, 1e-16;
        #  the display values come out the same to the last bit here, which is not promised: held to 1e-6 of the peak)
        assert rel_err(got[k][0], want[k][0]) < 1e-6, k
        assert abs(got[k][1] - want[k][1]) <= 1e-12 * abs(want[k][1]) and abs(got[k][2] - want[k][2]) <= 1e-12 * max(abs(want[k][2]), 1e-30), k
    one.close(); calls.close()
    # 2 blocks plain, 2 blocks with peak hold, 1 block plain again
    import oracle.ref_modems as RM
    if not (_backend() == "ref" and RM.spectrum_available()):
        return                                   # (the chain switch is checked against the reference's own class only)
    cpp = RM.RefSpectrumCpp(F, fs)
    cpp.set_center(0); cpp.set_bandwidth(fs)
    label = "reference class"
    sp = SpectrumProcessor(ctx, F, max_frames=10)
    worst, k, worst_hold, held = 0.0, 0, 0.0, 0
    for b in range(nb):
        if b == 2:
            sp.set_peak_hold(True); cpp.set_peak_hold(True)
        if b == 4:
            sp.set_peak_hold(False); cpp.set_peak_hold(False)
        n = sp.process(x[b * block:(b + 1) * block], 1, block, contiguous=True)
        for i in range(n):
            pts, ce, fl = sp.fetch(i)
            hold = sp.fetch_hold(i)
            wp, wce, wfl, whold = cpp.process(x[k * 2 * F:(k + 1) * 2 * F], 0, fs)
            worst = max(worst, rel_err(pts, wp))
            assert abs(ce - wce) <= TOL * abs(wce) and abs(fl - wfl) <= TOL * abs(wce), (b, i)       # (both on the ceiling's scale, as in _spectrum_contiguous_batches)
            assert (hold is None) == (whold is None), (b, i)
            if hold is not None:
                worst_hold = max(worst_hold, rel_err(hold, whold)); held += 1
            k += 1
    print("headline spectrum across peak-hold switches (%s): %d frames, worst points %.3g, %d held lines, worst %.3g" % (label, k, worst, held, worst_hold))
    assert worst < TOL and worst_hold < TOL and held >= 10
    sp.close(); cpp.close()
    # another averaging rate and scale factor through the fused chain (setFFTAverageRate / setScaleFactor)
    cpp = RM.RefSpectrumCpp(F, fs)
    cpp.set_center(0); cpp.set_bandwidth(fs); cpp.set_average_rate(0.3); cpp.set_scale(2.5)
    sp = SpectrumProcessor(ctx, F, max_frames=20)
    sp.set_average_rate(0.3); sp.set_scale_factor(2.5)
    n = sp.process(x[:2 * block], 2, block, contiguous=True)
    worst = 0.0
    for i in range(n):
        pts, ce, fl = sp.fetch(i)
        wp, wce, wfl, _ = cpp.process(x[i * 2 * F:(i + 1) * 2 * F], 0, fs)
        worst = max(worst, rel_err(pts, wp))
        assert abs(ce - wce) <= TOL * abs(wce) and abs(fl - wfl) <= TOL * abs(wce), i
    print("headline spectrum, rate 0.3, scale 2.5: %d frames, worst points %.3g" % (n, worst))
    assert worst < TOL
    sp.close(); cpp.close()


def test_spectrum_size_that_is_not_a_power_of_two_contiguous_batches(ctx):
    """fftSize 600 (1200-point transforms) and 375 (odd: the two bins of a display point straddle the fftshift's wrap), contiguous frames over
    three calls against the reference's own class: averagers, trackers, carry"""
    _spectrum_contiguous_batches(ctx, 600, 2400000, (30, 22, 25))
    _spectrum_contiguous_batches(ctx, 375, 2400000, (12, 9, 14))


def test_spectrum_large_size_that_is_not_a_power_of_two_contiguous_batches(ctx):
    """fftSize 1500 and 3000 (3000- and 6000-point transforms: convolutions of 8192 and 16384 points, one and two radix passes in front of the
    4096-point rows) and 20000 (40000 points through a 131072-point convolution), contiguous frames over three calls against the reference's class"""
    _spectrum_contiguous_batches(ctx, 1500, 2400000, (14, 9, 11))
    _spectrum_contiguous_batches(ctx, 3000, 2400000, (9, 7, 8))
    _spectrum_contiguous_batches(ctx, 20000, 10000000, (4, 3, 5))


def _spectrum_contiguous_batches(ctx, F, fs, frames_per_batch, against_exact=False):
    """The BASELINE spectrum shapes as the bench runs them: F = 65536 (C3: 32 rows of 4096 behind a radix-32 pass) and F = 16384 (C2),
    CSDR_SPEC_CONTIGUOUS, >= 300 frames per call (several 256-frame rounds of the averaging scan, multi-row tiles), three consecutive
    batches carrying the averagers, the ceiling / floor trackers and a partial frame (the batches are NOT whole multiples of 2F) from
    one call to the next, input resident in HBM.  EVERY frame is compared with the reference processor fed the same frames one
    process() at a time: points at 1e-5 of the frame's peak, ceiling / floor at 1e-5 (SpectrumVisualProcessor.cpp:387-576, :626-627)."""
    from cubicsdr_amd.engine import SpectrumProcessor
    try:
        import torch
        dev = torch.device("cuda", 0) if torch.cuda.is_available() else None
    except Exception:
        dev = None
    N = 2 * F
    odd = (1000 % N, 77 % N, (N - 1077) % N)                           # samples left over after the last whole frame of each call
    lens = [nf * N + o for nf, o in zip(frames_per_batch, odd)]
    lens[1] -= odd[0]; lens[2] -= odd[1]                               # call k starts with the carry of call k - 1
    total = sum(lens)
    carriers = [("NBFM", 0.21 * fs), ("AM", -0.33 * fs), ("USB", 0.05 * fs), ("NBFM", -0.07 * fs)]
    x = synth_iq_fast(total, fs, 0, carriers, seed=4242)
    # slow fade so that ceiling / floor trackers and the averagers keep moving over the ~1000 frames
    nfr = -(-total // N)
    env = np.repeat((1.0 + 0.6 * np.sin(np.arange(nfr) * 0.05)).astype(np.float32), N)[:total]
    x *= env
    del env
    x = np.ascontiguousarray(x, dtype=np.complex64)
    step, kind = _ref_spectrum_frames(F, fs)
    exact = None
    if against_exact:
        # A display value is log10(maa + 1 - floor) / log10(ceil + 1 - floor) (:562): for the weakest bins its slope is 0.076 per unit of ABSOLUTE
        # magnitude error, and a float32 transform of 2^21 points carries an absolute error of 1.6e-4 rms per bin (liquid's and this one alike:
        # profiles/experiments/spectrum_2m_sensitivity.py), i.e. 1e-5 .. 4e-5 of display value: at this size the reference itself is not within
        # 1e-5 of the exact result.  So the same frames also go through the restatement with a FLOAT64 transform, and the HIP path has to be as
        # close to that as the reference's own class is (and within TOL + both distances of the reference).
        exact = exact_spectrum(_backend(), F)
    sp = SpectrumProcessor(ctx, F, max_frames=max(frames_per_batch) + 1)
    pos = done = 0
    worst = worst_c = worst_ref_exact = worst_hip_exact = 0.0
    for k, n in enumerate(lens):
        xd = torch.from_numpy(x[pos:pos + n].view(np.float32).reshape(-1, 2)).to(dev) if dev is not None else x[pos:pos + n]
        nf = sp.process(xd, 1, n, contiguous=True)
        expect = (pos + n) // N - done
        assert nf == expect, (k, nf, expect)
        for j in range(nf):
            wp, wce, wfl = step(x[(done + j) * N:(done + j + 1) * N])
            pts, ce, fl = sp.fetch(j)
            e = rel_err(pts, wp)
            worst = max(worst, e)
            worst_c = max(worst_c, abs(ce - wce) / abs(wce), abs(fl - wfl) / abs(wce))
            if exact is not None:
                ep, ece, efl = exact.process_frame(x[(done + j) * N:(done + j + 1) * N])
                e_ref, e_hip = rel_err(wp, ep), rel_err(pts, ep)
                worst_ref_exact, worst_hip_exact = max(worst_ref_exact, e_ref), max(worst_hip_exact, e_hip)
                assert e_hip < max(TOL, 1.5 * e_ref), (k, j, e_hip, e_ref)
                assert e < TOL + e_ref + e_hip, (k, j, e, e_ref, e_hip)
            else:
                assert e < TOL, (k, j, e)
            assert abs(ce - wce) <= TOL * abs(wce) and abs(fl - wfl) <= TOL * abs(wce), (k, j, ce, wce, fl, wfl)
        done += nf
        pos += n
        del xd
    assert done == total // N
    print("spectrum F=%d (%s): %d frames, worst points %.3g, worst ceiling/floor %.3g" % (F, kind, done, worst, worst_c))
    if exact is not None:
        print("   against the float64 transform: reference %.3g, HIP path %.3g" % (worst_ref_exact, worst_hip_exact))
    sp.close()


@pytest.mark.parametrize("F,frames,nan_at", [(2048, (40, 23), ((5, 100), (38, 7), (41, 3000))), (4096, (300,), ((17, 9), (255, 0), (256, 11), (290, 5000)))])
def test_spectrum_nan_samples_recover_frame_by_frame(ctx, F, frames, nan_at):
    """A NaN IQ sample makes every magnitude of its frame NaN; the reference repairs its averagers frame by frame (SpectrumVisualProcessor.cpp
    :494-497: `if (maa != maa) maa = x; ... if (ma != ma) ma = x`) and shows finite points again two frames later.  The averaging kernel is a
    blocked scan over frame groups; a round that holds a non-finite magnitude takes the frame-ordered path with the same statements.  NaN
    frames at the start / inside / at the end of a frame group, at a 256-frame round boundary and in the last frames of a call (the NaN state
    is carried into the next call): the NaN masks of the points are identical, every finite point, ceiling and floor within 1e-5."""
    from cubicsdr_amd.engine import SpectrumProcessor
    N = 2 * F
    fs = 2400000
    total = sum(frames) * N
    x = synth_iq(total, fs, 0, [("NBFM", 300000.0), ("AM", -500000.0)], seed=77)
    for fr, off in nan_at:
        x[fr * N + off] = np.complex64(complex(np.nan, 0.25))
    step, kind = _ref_spectrum_frames(F, fs)
    sp = SpectrumProcessor(ctx, F, max_frames=max(frames))
    done = nan_frames = 0
    for nfc in frames:
        nf = sp.process(x[done * N:(done + nfc) * N], 1, nfc * N, contiguous=True)
        assert nf == nfc
        for j in range(nf):
            wp, wce, wfl = step(x[(done + j) * N:(done + j + 1) * N])
            pts, ce, fl = sp.fetch(j)
            bad = np.isnan(wp)
            assert np.array_equal(np.isnan(pts), bad), (done + j, int(bad.sum()), int(np.isnan(pts).sum()))
            nan_frames += int(bad.any())
            if not bad.all():
                ok = ~bad
                assert rel_err(pts[ok], wp[ok]) < TOL, (done + j,)
            for g, w in ((ce, wce), (fl, wfl)):
                assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= TOL * abs(wce), (done + j, ce, wce, fl, wfl)
        done += nf
    assert nan_frames >= len(nan_at)
    print("spectrum with NaN samples (%s): %d frames, %d of them with NaN points, as in the reference" % (kind, done, nan_frames))
    sp.close()


def test_pipelined_batches_equal_synchronised_batches(ctx):
    """The stage streams let consecutive batches overlap (channelizer of batch i+1 while the demodulators work on batch
    i; buffer rotations guarded by events).  Enqueue 6 batches back to back without touching the results, then compare the
    last batch's audio / spectrum bit for bit with a run that synchronises after every batch."""
    from cubicsdr_amd.engine import DemodBank, SDRPost, SpectrumProcessor
    fs, M, block, center, nbat, bpb = 2400000, 4, 40000, 100000000, 6, 2
    kinds = ["NBFM", "AM", "USB", "NBFM"]
    freqs = demod_frequencies(center, fs, len(kinds))
    bws = [12500, 6000, 5400, 12500]
    x = synth_iq(nbat * bpb * block, fs, center, list(zip(kinds, freqs)), seed=31)

    def run(sync_each):
        post = SDRPost(ctx, fs, M, block, max_blocks=bpb)
        bank = DemodBank(ctx, len(kinds), max_blocks=bpb)
        spec = SpectrumProcessor(ctx, 2048, max_frames=bpb)
        for i, (k, f) in enumerate(zip(kinds, freqs)):
            bank.configure(i, post, k, bws[i], f)
        for b in range(nbat):
            xb = x[b * bpb * block:(b + 1) * bpb * block]
            post.execute(xb, bpb, block, center)
            bank.execute(post)
            spec.process(xb, bpb, block)
            if sync_each:
                ctx.synchronize()
        out = [bank.audio(i) for i in range(len(kinds))] + [bank.iq(i) for i in range(len(kinds))]
        out += [spec.fetch(k)[0] for k in range(bpb)] + [post.read_channel(ch) for ch in range(M)]
        res = [(r.n_iq, r.n_audio, r.level_accum, r.audio_peak) for i in range(len(kinds)) for r in bank.results(i)]
        spec.close(); bank.close(); post.close()
        return out, res

    a, ra = run(True)
    for _ in range(3):
        b, rb = run(False)
        assert ra == rb
        for u, v in zip(a, b):
            assert np.array_equal(u, v)


# ----------------------------------------------------------------------------------------------- BASELINE config shapes
def test_c3_shape_mixed_m122(ctx):
    """BASELINE config 3 (the headline): 61.44 MS/s, M = 122 (channel rate 503606 by integer division), block 1 024 068, ALL 256
    mixed NBFM / AM / USB demodulators over 3 consecutive blocks against the oracle, as one batch and block at a time."""
    hist = np.zeros(_ERR_EDGES.size - 1, np.int64)
    per = []
    print("c3 worst errors", _full_config(ctx, 61440000, 122, 1024068, ["NBFM", "AM", "USB"] * 85 + ["NBFM"], 3, seed=41, hist=hist, persample=per))
    # the margin of the worst sample is thin (the reference's own sensitivity); the distribution behind that maximum:
    print("c3 audio, per-sample |gpu - reference| / peak of the demodulator, %d samples:" % hist.sum())
    for lo, hi, n in zip(_ERR_EDGES[:-1], _ERR_EDGES[1:], hist):
        print("   [%.0e, %s): %9d  (%.5f %%)" % (lo, "%.0e" % hi if hi < 1 else "inf", n, 100.0 * n / max(1, hist.sum())))
    assert hist[-1] == 0
    per = np.concatenate(per)
    print("c3 audio, per-sample |gpu - reference| / max(|reference sample|, 1 % of the demodulator's peak): " +
          ", ".join("p%s %.2e" % (q, np.percentile(per, float(q))) for q in ("50", "90", "99", "99.9", "99.99", "100")))


def test_c3n_shape_all_nbfm_m122(ctx):
    """the north-star wording of config 3: 256 NBFM demodulators behind the M = 122 channelizer, 3 blocks, every demodulator."""
    print("c3n worst errors", _full_config(ctx, 61440000, 122, 1024068, ["NBFM"] * 256, 3, seed=43))


def test_c4_shape_m1024_channelizer_and_nbfm(ctx):
    """BASELINE config 4 shape: 100 MS/s, firpfbch M = 1024 (32 x 32 two-step DFT path, FIR straight from HBM), NBFM on a
    97 656 S/s channel (two half-band stages: the generic front-end kernel)."""
    from cubicsdr_amd.engine import SDRPost
    from oracle.cubicsdr_chain import RefSDRPost
    fs, M, block, center = 100000000, 1024, 1667072, 400000000
    x = synth_iq(block, fs, center, [("NBFM", center + 1234567), ("NBFM", center - 33000000)], seed=51)
    ref = RefSDRPost(_backend(), fs, M)
    post = SDRPost(ctx, fs, M, block, max_blocks=1)
    ref.run_block(x, center)
    post.execute(x, 1, block, center)
    for ch in (0, 1, 13, 511, 512, 513, 686, 1023, 1024):
        want, fc, rate = ref.channel_data(ch)
        got = post.read_channel(ch)
        assert post.channel_center(ch) == fc
        if ch == 0:
            # the analyzer has DC gain M, so channel 0 carries 0.01 * 1024 and the reference's float32 DC-blocker state
            # sits near 10.24 / 0.0005 = 20480: its own rounding noise (see test_dc_blocker_large_offset_state_noise)
            floor = 4 * np.spacing(np.float32(0.01 * M / 0.0005))
            assert np.max(np.abs(got - want)) < TOL * np.max(np.abs(want)) + floor
        else:
            assert rel_err(got, want) < TOL, ch
    post.close()


def test_c4_full_size_all_1024_demodulators(ctx):
    """BASELINE config 4 at full size: one NBFM demodulator on EVERY one of the 1024 channels, three 1 667 072-sample blocks, as one
    batch and block at a time; every demodulator's resampled IQ / audio / level / peak against the reference chain, counts and phase
    words exact (SDRPostThread.cpp:303-398 routing, DemodulatorPreThread.cpp:154-220, ModemNBFM.cpp:36)."""
    w = _full_config(ctx, 100000000, 1024, 1667072, ["NBFM"] * 1024, 3, seed=52)
    print("c4 full size (1024 NBFM x 3 blocks) worst errors", w)


def test_c5_shape_m200_and_1m_point_spectrum(ctx):
    """BASELINE config 5 shape: 100 MS/s, M = 200, block 1 666 800; spectrum fftSize 1 048 576 (internal 2^21 points:
    radix-16 and radix-32 passes in front of the 4096-point rows)."""
    from cubicsdr_amd.engine import SDRPost, SpectrumProcessor
    from oracle.cubicsdr_chain import RefSDRPost, RefSpectrum
    fs, M, block, center = 100000000, 200, 1666800, 400000000
    x = synth_iq(2 * block, fs, center, [("NBFM", center + 7654321), ("AM", center - 21000000)], seed=61)
    ref = RefSDRPost(_backend(), fs, M)
    post = SDRPost(ctx, fs, M, block, max_blocks=1)
    ref.run_block(x[:block], center)
    post.execute(x[:block], 1, block, center)
    for ch in (0, 15, 99, 100, 158, 199, 200):
        want, fc, rate = ref.channel_data(ch)
        got = post.read_channel(ch)
        if ch == 0:     # DC gain M: the reference's float32 DC-blocker state noise, as in the M = 1024 test
            assert np.max(np.abs(got - want)) < TOL * np.max(np.abs(want)) + 4 * np.spacing(np.float32(0.01 * M / 0.0005))
        else:
            assert rel_err(got, want) < TOL, ch
    post.close()
    F = 1 << 20
    sp = SpectrumProcessor(ctx, F, max_frames=2)
    rs = RefSpectrum(_backend(), F)
    assert rel_err(sp.fft_only(x[:2 * F]), rs.fft(x[:2 * F])) < TOL
    assert sp.process(x, 2, block, contiguous=True) == 1        # 3 333 600 samples hold one 2 097 152-point frame
    pts, ce, fl = sp.fetch(0)
    wp, wce, wfl = rs.process_frame(x[:2 * F])
    assert rel_err(pts, wp) < TOL
    assert abs(ce - wce) <= TOL * abs(wce) and abs(fl - wfl) <= TOL * abs(wce)
    sp.close()


def test_c5_full_size_all_512_demodulators(ctx):
    """BASELINE config 5's per-GPU workload at full size: 512 mixed NBFM / AM / USB demodulators behind the M = 200 channelizer
    (500 kS/s channels), three 1 666 800-sample blocks, batched and block at a time."""
    kinds = (["NBFM", "AM", "USB"] * 171)[:512]
    w = _full_config(ctx, 100000000, 200, 1666800, kinds, 3, seed=62)
    print("c5 full size (512 mixed x 3 blocks) worst errors", w)


def test_c5_spectrum_32_frames_of_2m_points_across_calls(ctx):
    """The C5 spectrum as the bench runs it: fftSize 1 048 576 (2^21-point transforms: radix-16 and radix-32 passes in front of the
    4096-point rows), contiguous frames, 12 + 11 + 9 frames over three calls with the averagers, ceiling / floor trackers and a partial
    frame carried from call to call; EVERY frame against the reference's own SpectrumVisualProcessor
    (SpectrumVisualProcessor.cpp:387-576) AND against the same arithmetic with a float64 transform (see _spectrum_contiguous_batches:
    at 2^21 points "1e-5 of the peak" lies below the float32 transforms' own noise in the weakest bins)."""
    _spectrum_contiguous_batches(ctx, 1 << 20, 100000000, (12, 11, 9), against_exact=True)


def test_active_channel_subset_matches_all_channels(ctx):
    """csdr_post_set_active_channels (the channels with consumers, SDRPostThread.cpp:336-339; what a demodulator-sharded rank
    produces): the rows of the active channels equal the all-channels run bit for bit, the other rows are not written, and a
    demodulator routed to an inactive channel is refused."""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    from cubicsdr_amd.hip import CsdrError
    for fs, M, block in ((10000000, 20, 166680), (61440000, 122, 122 * 300)):
        center = 100000000
        x = synth_iq(4 * block, fs, center, [("NBFM", center + 1234567)], seed=81)
        full = SDRPost(ctx, fs, M, block, max_blocks=1)
        part = SDRPost(ctx, fs, M, block, max_blocks=1)
        active = sorted({0, 3, M // 2, M - 1, 7 % M})
        part.set_active_channels(active)
        sentinel = None
        for b in range(4):
            full.execute(x[b * block:(b + 1) * block], 1, block, center)
            part.execute(x[b * block:(b + 1) * block], 1, block, center)
            for ch in range(M):
                if ch in active:
                    assert np.array_equal(part.read_channel(ch), full.read_channel(ch)), (M, b, ch)
            if b not in (0, 3):                                   # the output buffers rotate (three of them when the channelizer has
                continue                                          # its own stream): blocks 0 and 3 land in the same one either way
            rows = {ch: part.read_channel(ch) for ch in range(M) if ch not in active}
            if sentinel is None:
                sentinel = rows                                   # whatever the buffer held: it must not change any more
            else:
                for ch, r in rows.items():
                    assert np.array_equal(r, sentinel[ch], equal_nan=True), (M, ch)
        # a demodulator on an inactive channel: refused, and nothing else disturbed
        bank = DemodBank(ctx, 2, max_blocks=1)
        f_inactive = part.channel_center(1) + 1000
        bank.configure(0, part, "NBFM", 12500, f_inactive)
        with pytest.raises(CsdrError):
            bank.execute(part)
        bank.set_frequency(0, part.channel_center(3) + 1000)
        bank.execute(part)
        assert bank.results(0)[0].n_iq > 0
        part.set_active_channels(None)                             # back to every channel
        part.execute(x[:block], 1, block, center)
        bank.close(); full.close(); part.close()


def test_sharded_stream_equals_unsharded(ctx):
    """BASELINE config 4 partitioning on one GPU: two "virtual ranks" (two contexts, disjoint demodulator shards, each
    channelizing only the channels its own demodulators sit on) reproduce the unsharded audio of every demodulator bit for bit,
    and the host-side routing used for planning equals the library's."""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    from cubicsdr_amd.parallel import ShardedStream, channel_at, data_channel
    fs, M, block, center, nb = 100000000, 1024, 1667072, 400000000, 2
    nd = 48
    freqs = demod_frequencies(center, fs, nd)
    demods = [("NBFM", 12500, f) for f in freqs]
    x = synth_iq_fast(nb * block, fs, center, [("NBFM", f) for f in freqs[:8]], seed=91)
    post = SDRPost(ctx, fs, M, block, max_blocks=nb)
    bank = DemodBank(ctx, nd, max_blocks=nb)
    for i, (k, bw, f) in enumerate(demods):
        bank.configure(i, post, k, bw, f)
    post.execute(x, nb, block, center)
    for k, bw, f in demods:                                      # (the library knows the stream's centre frequency from the first block on)
        assert channel_at(f, center, fs, M) == post.channel_at(f)
    bank.execute(post)
    whole = [bank.audio(i) for i in range(nd)]
    counts = [[(r.n_iq, r.n_audio, r.nco_theta, r.resamp_phase) for r in bank.results(i)] for i in range(nd)]
    bank.close(); post.close()
    import torch
    xd = torch.from_numpy(x.view(np.float32).reshape(-1, 2)).cuda()
    ranks = [ShardedStream(0, r, 2, fs, M, block, demods, center, nb, group=False) for r in range(2)]
    assert sorted(ranks[0].plan.demods + ranks[1].plan.demods) == list(range(nd))
    assert not (set(ranks[0].plan.active_channels) & set(ranks[1].plan.active_channels))
    assert all(len(r.plan.active_channels) < M // 8 for r in ranks)            # each rank computes a small subset of the 1024 rows
    for r in ranks:
        r.step(xd, nb)
    for r in ranks:
        for i in r.plan.demods:
            assert np.array_equal(r.audio(i), whole[i]), i
            assert [(q.n_iq, q.n_audio, q.nco_theta, q.resamp_phase) for q in r.results(i)] == counts[i], i
        r.close()


def _slab_case(ctx, fs, M, block, nd, n_batches, nb, world, use_torch, kinds=("NBFM",)):
    """ONE stream sharded by time for the channelizer and by channel for the demodulators (parallel.SlabStream), `world` virtual ranks in
    this process with the all-to-all done by slicing: every demodulator's audio and counts must equal the unsharded path's over
    n_batches consecutive batches of nb blocks (the polyphase windows, channel 0's DC blocker and every demodulator state carry
    across slabs AND batches).  A demodulator sits on channel 0 so that the deferred DC blocker is exercised."""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    from cubicsdr_amd.parallel import SlabStream, local_exchange, slab_blocks
    center = 400000000
    freqs = demod_frequencies(center, fs, nd)
    freqs[0] = center + 1500                                     # channel 0 (the DC-blocked row)
    bw = {"NBFM": 12500, "AM": 6000, "USB": 5400}
    demods = [(kinds[i % len(kinds)], bw[kinds[i % len(kinds)]], f) for i, f in enumerate(freqs)]
    x = synth_iq(n_batches * nb * block, fs, center, [(k, f) for k, _, f in demods[:6]], seed=97)
    post = SDRPost(ctx, fs, M, block, max_blocks=nb)
    bank = DemodBank(ctx, nd, max_blocks=nb)
    for i, (k, b, f) in enumerate(demods):
        bank.configure(i, post, k, b, f)
    whole, counts = [], []
    for t in range(n_batches):
        post.execute(x[t * nb * block:(t + 1) * nb * block], nb, block, center)
        bank.execute(post)
        whole.append([bank.audio(i) for i in range(nd)])
        counts.append([[(r.n_iq, r.n_audio, r.nco_theta, r.resamp_phase) for r in bank.results(i)] for i in range(nd)])
    bank.close(); post.close()
    ranks = [SlabStream(0, r, world, fs, M, block, demods, center, nb, group=False, use_torch=use_torch) for r in range(world)]
    assert sorted(sum((r.plan.demods for r in ranks), [])) == list(range(nd))
    assert sum(c for _, c in slab_blocks(nb, world)) == nb
    xf = x.view(np.float32).reshape(-1, 2)
    worst = 0.0
    for t in range(n_batches):
        batch = xf[t * nb * block:(t + 1) * nb * block]
        if use_torch:
            import torch
            batch = torch.from_numpy(batch.copy()).cuda()
        ext = ranks[0].extended(batch, nb)                      # the ingest rank's [history | batch]
        sends = [r.produce(r.window(ext, nb, r.rank), nb) for r in ranks]
        recvs = local_exchange(ranks, sends, nb)
        for r, rv in zip(ranks, recvs):
            r.consume(rv, nb)
        for r in ranks:
            for i in r.plan.demods:
                got = r.audio(i)
                assert [(q.n_iq, q.n_audio, q.nco_theta, q.resamp_phase) for q in r.results(i)] == counts[t][i], (t, i)
                assert got.shape == whole[t][i].shape, (t, i)
                if not np.array_equal(got, whole[t][i]):
                    worst = max(worst, rel_err(got, whole[t][i]))
    for r in ranks:
        r.close()
    # rows are bit-identical except channel 0's, whose DC blocker scans tiles of another size (fp64 blocked scan: last-bit differences)
    assert worst < 1e-6, worst
    return worst


def test_time_slab_sharding_equals_unsharded(ctx):
    """SURVEY 8e option 2 on one GPU: 2 and 3 virtual ranks (3 does not divide the 4 blocks of a batch: uneven slabs), M = 64 channelizer,
    24 mixed demodulators, 2 consecutive batches."""
    print("slab worst", _slab_case(ctx, 6400000, 64, 106688, 24, 2, 4, 2, True, kinds=("NBFM", "AM", "USB")),
          _slab_case(ctx, 6400000, 64, 106688, 24, 2, 4, 3, True))


def _comm_one_rank_case(ctx, use_torch):
    """The C ABI's communicator (csdr_comm: RCCL, loaded on first use) with ONE rank: every collective entry point runs on the boundary stream
    (ncclCommInitRank with one rank; the host-executing test build copies instead) and the two sharded drivers, given a communicator id,
    go through csdr_comm_broadcast / csdr_comm_scatter / csdr_post_exchange_rows: audio and counts equal the unsharded path's."""
    from cubicsdr_amd.engine import Comm, Context, DemodBank, SDRPost
    from cubicsdr_amd.parallel import ShardedStream, SlabStream, exchange_id
    fs, M, block, nd, nb, n_batches, center = 6400000, 64, 64 * 417, 12, 4, 2, 400000000
    freqs = demod_frequencies(center, fs, nd)
    freqs[0] = center + 1500
    kinds = ("NBFM", "AM", "USB")
    bw = {"NBFM": 12500, "AM": 6000, "USB": 5400}
    demods = [(kinds[i % 3], bw[kinds[i % 3]], f) for i, f in enumerate(freqs)]
    x = synth_iq(n_batches * nb * block, fs, center, [(k, f) for k, _, f in demods[:6]], seed=197)
    xf = x.view(np.float32).reshape(-1, 2)

    def dev(a):
        if not use_torch:
            return a.copy()
        import torch
        return torch.from_numpy(a.copy()).cuda()

    def host(t):
        return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    post = SDRPost(ctx, fs, M, block, max_blocks=nb)
    bank = DemodBank(ctx, nd, max_blocks=nb)
    for i, (k, b, f) in enumerate(demods):
        bank.configure(i, post, k, b, f)
    whole, counts = [], []
    for t in range(n_batches):
        post.execute(x[t * nb * block:(t + 1) * nb * block], nb, block, center)
        bank.execute(post)
        whole.append([bank.audio(i) for i in range(nd)])
        counts.append([[(r.n_iq, r.n_audio, r.nco_theta, r.resamp_phase) for r in bank.results(i)] for i in range(nd)])
    bank.close(); post.close()
    # (a communicator id serves ONE communicator: each object below gets its own)
    cid = exchange_id(0, 1)
    assert len(cid) == Comm.ID_BYTES
    # the bare collectives
    c2 = Context(0)
    comm = Comm(c2, cid, 0, 1)
    assert (comm.rank, comm.world) == (0, 1)
    a = dev(xf[:5000]); b = dev(np.zeros((5000, 2), np.float32)); c = dev(np.zeros((5000, 2), np.float32))
    comm.broadcast(a, 5000, 0)
    comm.scatter(a, b, 5000, 0)
    comm.all_to_all(b, [5000], c, [5000])
    assert comm.max(3.25) == 3.25
    comm.barrier()
    assert np.array_equal(host(a), xf[:5000]) and np.array_equal(host(b), xf[:5000]) and np.array_equal(host(c), xf[:5000])
    comm.close(); c2.close()
    # broadcast variant
    sh = ShardedStream(0, 0, 1, fs, M, block, demods, center, nb, comm_id=exchange_id(0, 1))
    for t in range(n_batches):
        sh.step(dev(xf[t * nb * block:(t + 1) * nb * block]), nb, src=0)
        for i in range(nd):
            assert np.array_equal(sh.audio(i), whole[t][i]), (t, i)
            assert [(q.n_iq, q.n_audio, q.nco_theta, q.resamp_phase) for q in sh.results(i)] == counts[t][i], (t, i)
    sh.close()
    # time-slab variant: scatter + export / all-to-all / import in one ABI call
    sl = SlabStream(0, 0, 1, fs, M, block, demods, center, nb, use_torch=use_torch, comm_id=exchange_id(0, 1))
    worst = 0.0
    for t in range(n_batches):
        sl.step(sl.scatter(dev(xf[t * nb * block:(t + 1) * nb * block]), nb, src=0), nb)
        for i in range(nd):
            got = sl.audio(i)
            assert [(q.n_iq, q.n_audio, q.nco_theta, q.resamp_phase) for q in sl.results(i)] == counts[t][i], (t, i)
            if not np.array_equal(got, whole[t][i]):
                worst = max(worst, rel_err(got, whole[t][i]))
    sl.close()
    assert worst < 1e-6, worst
    return worst


def _slab_overlap_case(use_torch, n_batches=5):
    """step(overlap=True) of the time-slab stream -- csdr_post_exchange_rows_begin / _finish: the row transfers of a batch started before the
    previous batch is imported and demodulated -- against the one-call form, over five back-to-back batches on a one-rank communicator (real
    RCCL on the GPU box; the loopback of the host-executing build): audio and per-block counts bit for bit, with the windows scattered from the
    ingest rank and with every rank taking its window where it lies (local_window)."""
    from cubicsdr_amd.parallel import SlabStream, exchange_id
    fs, M, block, nd, nb, center = 6400000, 64, 64 * 417, 12, 4, 400000000
    freqs = demod_frequencies(center, fs, nd)
    freqs[0] = center + 1500
    kinds = ("NBFM", "AM", "USB")
    bw = {"NBFM": 12500, "AM": 6000, "USB": 5400}
    demods = [(kinds[i % 3], bw[kinds[i % 3]], f) for i, f in enumerate(freqs)]
    x = synth_iq(n_batches * nb * block, fs, center, [(k, f) for k, _, f in demods[:6]], seed=211)
    xf = x.view(np.float32).reshape(-1, 2)

    def dev(a):
        if not use_torch:
            return a.copy()
        import torch
        return torch.from_numpy(a.copy()).cuda()

    def run(overlap, local):
        sl = SlabStream(0, 0, 1, fs, M, block, demods, center, nb, use_torch=use_torch, comm_id=exchange_id(0, 1))
        out = []

        def collect():
            out.append(([sl.audio(i) for i in range(nd)], [[(q.n_iq, q.n_audio, q.nco_theta, q.resamp_phase) for q in sl.results(i)] for i in range(nd)]))
        ring = dev(xf[:nb * block])
        for t in range(n_batches):
            if local:
                window = sl.local_window(ring, nb)                  # the same batch again and again: its own end is the history in front of it
            else:
                window = sl.scatter(dev(xf[t * nb * block:(t + 1) * nb * block]), nb, src=0)
            sl.step(window, nb, overlap=overlap)
            if not overlap:
                collect()
            elif t > 0:
                assert sl.comm.exchanges_pending == 1
                collect()                                           # batch t - 1
        if overlap:
            sl.flush()
            assert sl.comm.exchanges_pending == 0
            collect()
        sl.close()
        return out
    for local in (False, True):
        a, b = run(False, local), run(True, local)
        assert len(a) == len(b) == n_batches
        for t in range(n_batches):
            assert a[t][1] == b[t][1], (local, t)
            for i in range(nd):
                assert np.array_equal(a[t][0][i], b[t][0][i]), (local, t, i)


def test_slab_exchange_overlapped_equals_one_call_form():
    _slab_overlap_case(True)


def test_comm_refuses_bad_arguments(ctx):
    """the communicator's entry points never half-apply a bad call: ranks outside the world, a rank's own part as a transfer, counts that do
    not match, null buffers and posts of another context come back as negative codes; the communicator keeps working afterwards."""
    import ctypes as C
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import Context, SDRPost
    from cubicsdr_amd.parallel import exchange_id
    L = H.lib()
    EINVAL = -1
    cid = exchange_id(0, 1)
    comm = C.c_void_p()
    assert L.csdr_comm_create(ctx.h, cid, 1, 1, C.byref(comm)) == EINVAL           # rank outside the world
    assert L.csdr_comm_create(ctx.h, cid, 0, 0, C.byref(comm)) == EINVAL
    assert L.csdr_comm_create(None, cid, 0, 1, C.byref(comm)) == EINVAL
    assert L.csdr_comm_create(ctx.h, cid, 0, 1, C.byref(comm)) == 0
    assert L.csdr_comm_rank(comm) == 0 and L.csdr_comm_world(comm) == 1 and L.csdr_comm_rank(None) == -1 and L.csdr_comm_world(None) == 0
    n = 4096
    buf = C.c_void_p(); out = C.c_void_p()
    assert L.csdr_dev_alloc(ctx.h, n * 8, C.byref(buf)) == 0 and L.csdr_dev_alloc(ctx.h, n * 8, C.byref(out)) == 0
    x = (np.arange(2 * n, dtype=np.float32) / n).astype(np.float32)
    assert L.csdr_dev_upload(ctx.h, buf, x.ctypes.data_as(C.c_void_p), x.nbytes) == 0
    assert L.csdr_comm_broadcast(comm, buf, n, 1) == EINVAL                        # root outside the world
    assert L.csdr_comm_broadcast(comm, None, n, 0) == EINVAL
    assert L.csdr_comm_broadcast(comm, buf, -1, 0) == EINVAL
    assert L.csdr_comm_scatter(comm, None, out, n, 0) == EINVAL                    # the root has nothing to send
    assert L.csdr_comm_scatter(comm, buf, out, n, 3) == EINVAL
    cnt = (C.c_int64 * 1)(n); other = (C.c_int64 * 1)(n - 1); neg = (C.c_int64 * 1)(-1)
    assert L.csdr_comm_all_to_all(comm, buf, cnt, out, other) == EINVAL            # a rank's counts to and from itself differ
    assert L.csdr_comm_all_to_all(comm, buf, neg, out, cnt) == EINVAL
    assert L.csdr_comm_all_to_all(comm, None, cnt, out, cnt) == EINVAL
    op = (H.P2pOp * 1)(H.P2pOp(0, 0, buf.value, n))
    assert L.csdr_comm_p2p(comm, op, 1) == EINVAL                                  # a rank's own part is never a transfer
    op[0].peer = 2
    assert L.csdr_comm_p2p(comm, op, 1) == EINVAL
    assert L.csdr_comm_p2p(comm, None, 1) == EINVAL and L.csdr_comm_p2p(comm, None, 0) == 0
    assert L.csdr_comm_max(comm, None) == EINVAL
    # posts of another context
    c2 = Context(0)
    p1, p2 = SDRPost(ctx, 800000, 8, 8 * 64, max_blocks=1), SDRPost(c2, 800000, 8, 8 * 64, max_blocks=1)
    chans = (C.c_int * 8)(*range(8)); nch = (C.c_int * 1)(8); f0 = (C.c_int64 * 1)(0); fr = (C.c_int64 * 1)(64)
    assert L.csdr_post_exchange_rows(comm, p1.h, p2.h, chans, nch, f0, fr, 1, 8 * 64, 100000000) == EINVAL
    assert L.csdr_post_exchange_rows(comm, p1.h, None, chans, nch, f0, fr, 1, 8 * 64, 100000000) == EINVAL
    nneg = (C.c_int * 1)(-8)
    assert L.csdr_post_exchange_rows(comm, p1.h, p1.h, chans, nneg, f0, fr, 1, 8 * 64, 100000000) == EINVAL
    p1.close(); p2.close(); c2.close()
    # ... and a valid call still works
    assert L.csdr_comm_scatter(comm, buf, out, n, 0) == 0
    v = C.c_double(2.5)
    assert L.csdr_comm_max(comm, C.byref(v)) == 0 and v.value == 2.5
    y = np.zeros_like(x)
    assert L.csdr_dev_download(ctx.h, y.ctypes.data_as(C.c_void_p), out, y.nbytes) == 0
    assert np.array_equal(x, y)
    L.csdr_comm_destroy(comm)
    assert L.csdr_dev_free(ctx.h, buf) == 0 and L.csdr_dev_free(ctx.h, out) == 0


@pytest.mark.parametrize("M", [10, 20, 68, 122])
def test_packed_row_order_holds_the_same_rows(ctx, M):
    """csdr_post_set_row_order (time-slab producers: rows grouped by owning rank, so that the output buffer is the all-to-all's send buffer):
    for a three-rank channel plan the packed post's rows -- read back by channel, and exported -- equal the plain post's bit for bit, in all
    three channelizer kernels (M = 10 / 122: chan_analyze_p2, 20: chan_analyze_fft, 68: chan_analyze); unlisted channels are refused."""
    from cubicsdr_amd.engine import SDRPost
    from cubicsdr_amd.hip import CsdrError
    fs, block, center = 500000 * M, M * 150, 100000000
    x = [synth_iq(block, fs, center, [("NBFM", center + 123456)], seed=5 + b, t0=b * block) for b in range(2)]
    plain = SDRPost(ctx, fs, M, block)
    packed = SDRPost(ctx, fs, M, block)
    plain.set_dc_blocker(False); packed.set_dc_blocker(False)
    owned = [[k for k in range(M) if k % 3 == q and k != 5] for q in range(3)]        # channel 5 has no owner
    order = [c for o in owned for c in o]
    packed.set_row_order(order)
    for b in range(2):
        plain.execute(x[b], 1, block, center)
        packed.execute(x[b], 1, block, center)
        for ch in order:
            assert np.array_equal(packed.read_channel(ch), plain.read_channel(ch)), (b, ch)
    with pytest.raises(CsdrError):
        packed.read_channel(5)
    packed.set_row_order(None)                                                       # back to row = channel, every channel produced
    packed.execute(x[1], 1, block, center)
    plain.execute(x[1], 1, block, center)
    assert np.array_equal(packed.read_channel(5), plain.read_channel(5))
    plain.close(); packed.close()


def test_comm_one_rank_through_the_abi(ctx):
    print("communicator, one rank: slab worst", _comm_one_rank_case(ctx, True))


def test_c2_full_size_batching_invariance(ctx):
    """Size-independent property at the full C2 size: 64 NBFM demodulators, 16 blocks -- the audio, the resampled IQ and
    the per-block counts of one 16-block batch equal, bit for bit, those of 16 one-block batches."""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    fs, M, block, center, nb, nd = 10000000, 20, 166680, 100000000, 16, 64
    freqs = demod_frequencies(center, fs, nd)
    x = synth_iq(nb * block, fs, center, [("NBFM", f) for f in freqs[:6]], seed=71)

    def run(batch):
        post = SDRPost(ctx, fs, M, block, max_blocks=batch)
        bank = DemodBank(ctx, nd, max_blocks=batch)
        for i, f in enumerate(freqs):
            bank.configure(i, post, "NBFM", 12500, f)
        audio = [[] for _ in range(nd)]
        counts = []
        for b0 in range(0, nb, batch):
            post.execute(x[b0 * block:(b0 + batch) * block], batch, block, center)
            bank.execute(post)
            for i in range(nd):
                audio[i].append(bank.audio(i))
                counts += [(r.n_iq, r.n_audio, r.level_count, r.nco_theta, r.resamp_phase, r.buffer_index) for r in bank.results(i)] if i < 4 else []
        post.close(); bank.close()
        return [np.concatenate(a) for a in audio], counts

    a1, c1 = run(nb)
    a2, c2 = run(1)
    assert sorted(c1) == sorted(c2)
    for u, v in zip(a1, a2):
        assert np.array_equal(u, v)


def test_retune_skip_and_inactive(ctx):
    """Control-flow edges of DemodulatorPreThread::run (:154-165): a demodulator that is retuned between blocks keeps its NCO
    phase and resampler state and only changes the phase increment; a demodulator tuned more than 0.75 x rate away from the
    block's centre skips blocks without touching its state; an inactive demodulator is not fed at all."""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    from oracle.cubicsdr_chain import RefDemod, RefSDRPost
    fs, block, center = 480000, 8000, 50000000           # single-channel mode: shifts can exceed the skip bound
    be = _backend()
    x = synth_iq(8 * block, fs, center, [("NBFM", center + 50000), ("AM", center - 120000)], seed=81)
    post, ref_post = SDRPost(ctx, fs, 1, block, max_blocks=1), RefSDRPost(be, fs, 1)
    bank = DemodBank(ctx, 3, max_blocks=1)
    plan = [  # per block: frequency of demod 0 (NBFM, stays on its carrier), frequency of demod 1 (AM), demod 2 active?
        (center + 50000, center - 120000, True), (center + 50000, center - 120000, True),
        (center + 51500, center - 120000, False), (center + 51500, center + 400000, False),      # retune; skip (|shift| > 360 k)
        (center + 49000, center + 400000, True), (center + 49000, center - 120000, True),
        (center + 50500, center - 119000, True), (center + 50000, center, True)]                  # retunes; zero shift (no mixing)
    kinds, bws = ["NBFM", "AM", "NBFM"], [12500, 6000, 12500]
    refs = []
    for i, k in enumerate(kinds):
        f0 = (plan[0][0], plan[0][1], center + 50000)[i]
        bank.configure(i, post, k, bws[i], f0)
        refs.append(RefDemod(be, k, bws[i], f0, fs))
    for b, (f0, f1, act2) in enumerate(plan):
        xb = x[b * block:(b + 1) * block]
        bank.set_frequency(0, f0); refs[0].frequency = f0
        bank.set_frequency(1, f1); refs[1].frequency = f1
        bank.set_active(2, act2)
        post.execute(xb, 1, block, center)
        bank.execute(post)
        ref_post.run_block(xb, center)
        data, fc, rate = ref_post.channel_data(0)
        for i in range(3):
            res = bank.results(i)
            if i == 2 and not act2:
                assert res == []
                continue
            riq = refs[i].pre(data, fc, rate)
            if riq is None:
                assert len(res) == 1 and res[0].skipped == 1 and res[0].n_audio == 0, (b, i)
                continue
            want = refs[i].demodulate(riq)
            r = res[0]
            assert r.skipped == 0 and r.n_iq == riq.size and r.n_audio == want["audio"].size, (b, i, r.n_iq, riq.size)
            assert rel_err(bank.iq(i), riq) < TOL, (b, i)
            assert rel_err(bank.audio(i), want["audio"]) < TOL, (b, i)
    post.close(); bank.close()


def test_routing_follows_centre_and_demodulator_retunes(ctx):
    """getChannelAt per block (SDRPostThread.cpp:128-139, :317-323) behind M = 4: the channel of a demodulator changes when the stream's centre
    frequency moves (every channel centre moves with it) and when the demodulator itself is retuned across channels; between such steps the
    routing of a batch is the cached one.  Each step against the reference's post thread + pre-thread + modem, one block per batch.  (No step
    lands on channel 0: its DC-blocker state noise has its own tests.)"""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    from oracle.cubicsdr_chain import RefDemod, RefSDRPost
    fs, M, block, center = 2400000, 4, 40000, 100000000
    be = _backend()
    cw = fs // M
    f_a, f_b = center + 450000, center - 1050000
    # a carrier at every offset from the stream centre a demodulator is ever tuned to (+-450 k, +-1050 k): no step demodulates bare noise
    x = synth_iq(8 * block, fs, center, [("NBFM", f_a), ("AM", f_b), ("NBFM", center + 1050000), ("AM", center - 450000)], seed=91)
    post, ref_post = SDRPost(ctx, fs, M, block, max_blocks=1), RefSDRPost(be, fs, M)
    bank = DemodBank(ctx, 2, max_blocks=1)
    steps = [  # (stream centre, frequency of demod 0, frequency of demod 1)        channels
        (center, f_a, f_b), (center, f_a, f_b),                                    # 1, 2 (cached on the second block)
        (center - cw, f_a, f_b), (center - cw, f_a, f_b),                          # the centre moves by one channel: 2 (the wrap channel), 3
        (center - cw, f_a - cw, f_b), (center - cw, f_a - cw, f_b),                # demod 0 retuned into the next channel: 1, 3
        (center, f_a, f_b + cw), (center, f_a, f_b)]                               # centre and both demodulators at once: 1, 3; then the first routing
    kinds, bws = ["NBFM", "AM"], [12500, 6000]
    refs = []
    for i, k in enumerate(kinds):
        bank.configure(i, post, k, bws[i], steps[0][1 + i])
        refs.append(RefDemod(be, k, bws[i], steps[0][1 + i], ref_post.chan_bw))
    seen = set()
    for b, (c0, f0, f1) in enumerate(steps):
        xb = x[b * block:(b + 1) * block]
        for i, f in enumerate((f0, f1)):
            bank.set_frequency(i, f); refs[i].frequency = f
        post.execute(xb, 1, block, c0)
        bank.execute(post)
        ref_post.run_block(xb, c0)
        for i, f in enumerate((f0, f1)):
            ch = ref_post.channel_at(f)
            assert ch != 0, (b, i)
            seen.add((i, ch))
            data, fc, rate = ref_post.channel_data(ch)
            res = bank.results(i)
            riq = refs[i].pre(data, fc, rate)
            assert riq is not None and len(res) == 1 and res[0].skipped == 0, (b, i)
            want = refs[i].demodulate(riq)
            assert res[0].n_iq == riq.size and res[0].n_audio == want["audio"].size, (b, i, res[0].n_iq, riq.size)
            assert rel_err(bank.iq(i), riq) < TOL, (b, i, ch)
            assert rel_err(bank.audio(i), want["audio"]) < TOL, (b, i, ch)
    assert len({c for i, c in seen if i == 0}) >= 2 and len({c for i, c in seen if i == 1}) >= 2, seen      # the routing really moved
    post.close(); bank.close()


# ----------------------------------------------------------------------------------------------- error behaviour
def test_error_codes_and_edge_inputs(ctx):
    """The ABI never throws and never falls back: bad arguments, state errors, capacity overruns and not-built features come
    back as negative codes with a message; nothing is half-applied (a following valid call still gives reference results)."""
    import ctypes as C
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import DemodBank, SDRPost, SpectrumProcessor
    from oracle.cubicsdr_chain import RefSpectrum
    L = H.lib()
    EINVAL, ESTATE, ERANGE, EUNSUP = -1, -4, -5, -6
    assert L.csdr_strerror(0) == b"ok" or L.csdr_strerror(0)
    post = C.c_void_p()
    assert L.csdr_post_create(ctx.h, C.byref(post)) == 0
    buf = np.zeros(64, np.complex64)
    assert L.csdr_post_execute(post, buf.ctypes.data_as(C.c_void_p), 0, 1, 40, 0) == ESTATE          # not configured
    assert L.csdr_post_configure(post, 2400000, 5, H.CSDR_POST_PFBCH, 40000, 1) in (EINVAL, EUNSUP)     # odd channel count
    assert L.csdr_post_configure(post, 2400000, 4, H.CSDR_POST_SINGLE, 40000, 1) == EINVAL             # SINGLE <=> one channel
    assert L.csdr_post_configure(post, 2400000, 4, 7, 40000, 1) == EINVAL                              # unknown mode
    assert L.csdr_post_configure(post, 2400000, 4, H.CSDR_POST_PFBCH, 40002, 1) == EINVAL              # block not a multiple of M
    assert L.csdr_post_configure(post, 2400000, 4, H.CSDR_POST_PFBCH, 40000, 2) == 0
    x = synth_iq(3 * 40000, 2400000, 0, [("NBFM", 300000.0)], seed=61)
    assert L.csdr_post_execute(post, x.ctypes.data_as(C.c_void_p), 0, 3, 40000, 0) == ERANGE           # more blocks than configured
    assert L.csdr_post_execute(post, x.ctypes.data_as(C.c_void_p), 0, 1, 40002, 0) == ERANGE           # block longer than configured
    assert L.csdr_post_execute(post, x.ctypes.data_as(C.c_void_p), 0, 1, 39998, 0) == EINVAL           # not a multiple of M
    assert L.csdr_post_execute(post, None, 0, 1, 40000, 0) == EINVAL
    assert b"" != L.csdr_last_error()
    n = C.c_int()
    out = np.zeros(8, np.complex64)
    assert L.csdr_post_execute(post, x.ctypes.data_as(C.c_void_p), 0, 2, 40000, 0) == 0
    assert L.csdr_post_read_channel(post, 0, out.ctypes.data_as(C.c_void_p), 8, C.byref(n)) == ERANGE  # needs 20000 samples
    assert L.csdr_post_read_channel(post, 9, out.ctypes.data_as(C.c_void_p), 8, C.byref(n)) == EINVAL
    # bank: slot range, unknown modem, an unsupported rate combination
    bank = C.c_void_p()
    assert L.csdr_bank_create(ctx.h, 2, 2, C.byref(bank)) == 0
    prm = H.DemodParams(H.CSDR_MODEM_NBFM, 12500, 48000, 0, 300000)
    assert L.csdr_bank_configure_slot(bank, 5, C.byref(prm), post) == EINVAL
    bad = H.DemodParams(17, 12500, 48000, 0, 300000)
    assert L.csdr_bank_configure_slot(bank, 0, C.byref(bad), post) == EUNSUP
    wide = H.DemodParams(H.CSDR_MODEM_FM, 900000, 48000, 0, 300000)                 # bandwidth above the channel rate: the interpolating resampler
    assert L.csdr_bank_configure_slot(bank, 0, C.byref(wide), post) == 0
    up = H.DemodParams(H.CSDR_MODEM_FMS, 100000, 192000, 0, 300000)                 # FM stereo whose audio resamplers interpolate (round 3: supported)
    assert L.csdr_bank_configure_slot(bank, 0, C.byref(up), post) == 0
    assert L.csdr_bank_configure_slot(bank, 0, C.byref(prm), post) == 0
    res = (H.BlockResult * 1)()
    assert L.csdr_bank_execute(bank, post) == 0
    assert L.csdr_bank_fetch_results(bank, 0, res, 1, C.byref(n)) == ERANGE                            # two blocks, room for one
    # a demodulator outside the span: routed nowhere, no blocks (updateActiveDemodulators would have parked it)
    assert L.csdr_bank_set_frequency(bank, 0, 50000000) == 0
    assert L.csdr_bank_execute(bank, post) == 0
    res2 = (H.BlockResult * 2)()
    assert L.csdr_bank_fetch_results(bank, 0, res2, 2, C.byref(n)) == 0 and (n.value == 0 or all(r.skipped for r in res2[:n.value]))
    L.csdr_bank_destroy(bank)
    L.csdr_post_destroy(post)
    # spectrum: sizes, modes, capacity; a rejected call leaves the averagers untouched
    spec = C.c_void_p()
    assert L.csdr_spec_create(ctx.h, C.byref(spec)) == 0
    assert L.csdr_spec_process(spec, x.ctypes.data_as(C.c_void_p), 0, 1, 4096, 0) == ESTATE
    assert L.csdr_spec_setup(spec, 3000000, 4) == EUNSUP                                               # not a power of two: the chirp-z convolution would exceed 2^22 points
    assert L.csdr_spec_setup(spec, 1 << 22, 4) == EUNSUP                                               # internal transform above 2^22 points
    assert L.csdr_spec_setup(spec, 512, 0) == EINVAL
    assert L.csdr_spec_setup(spec, 512, 4) == 0
    assert L.csdr_spec_process(spec, x.ctypes.data_as(C.c_void_p), 0, 1, 4096, 9) == EINVAL            # unknown mode
    assert L.csdr_spec_process(spec, x.ctypes.data_as(C.c_void_p), 0, 1, 600, H.CSDR_SPEC_FIRST_FRAME) == EINVAL   # short input needs LINES
    assert L.csdr_spec_process(spec, x.ctypes.data_as(C.c_void_p), 0, 1, 2000, H.CSDR_SPEC_LINES) == EINVAL        # long input is not a line
    assert L.csdr_spec_process(spec, x.ctypes.data_as(C.c_void_p), 0, 9, 1024, H.CSDR_SPEC_CONTIGUOUS) == ERANGE   # 9 frames > max_frames
    pts = np.zeros(1024, np.float32)
    ce, fl = C.c_double(), C.c_double()
    assert L.csdr_spec_fetch(spec, 0, pts.ctypes.data_as(C.c_void_p), 1024, C.byref(ce), C.byref(fl)) == EINVAL   # no frame yet
    assert L.csdr_spec_process(spec, x.ctypes.data_as(C.c_void_p), 0, 1, 1024, H.CSDR_SPEC_FIRST_FRAME) == 0
    assert L.csdr_spec_fetch(spec, 0, pts.ctypes.data_as(C.c_void_p), 100, C.byref(ce), C.byref(fl)) == ERANGE
    assert L.csdr_spec_fetch(spec, 0, pts.ctypes.data_as(C.c_void_p), 1024, C.byref(ce), C.byref(fl)) == 0
    ref = RefSpectrum(_backend(), 512)
    wp, wce, wfl = ref.process_frame(x[:1024])
    assert rel_err(pts, wp) < TOL and abs(ce.value - wce) <= TOL * abs(wce)
    L.csdr_spec_destroy(spec)
