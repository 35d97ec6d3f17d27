"""The squelch bank on the device: the cases the emulation runs (tests/squelch_cases.py) against the checker at one float32 ulp, and what only the
device path has -- csdr_squelch_process_bank behind a running pipeline (the checker fed the bank's own csdr_bank_fetch_results sums), the gated
mixer feed against a second mixer fed the open blocks one by one, the recorder against csdr_bank_fetch_pcm16 cut by the flags, an execute issued
straight behind process_bank with no synchronise between, a stale execute, and one shape at size (256 slots x 128 blocks)."""
import numpy as np
import pytest

import cubicsdr_amd.hip as H
from oracle.cubicsdr_chain import RefLevelSquelch
from tests import squelch_cases as K
from tests.util import demod_frequencies, synth_iq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n_slots", K.SHAPES)
def test_squelch_against_the_checker(ctx, n_slots):
    n = K.check_scenario(ctx, n_slots, exact=False)
    assert n == n_slots * sum(K.CALLS) - K.CALLS[K.ABSENT[1]]


def test_squelch_against_the_reference_thread(ctx):
    import oracle.ref_modems as RM
    if not RM.demodthread_available():
        pytest.skip("oracle/_ref/libref_demodthread.so is built only where the reference is")
    assert K.check_against_demodthread(ctx, exact=False) == 168


def test_squelch_refusals(ctx):
    from cubicsdr_amd.engine import Context, DemodBank
    other = Context(0)
    bank, other_bank = DemodBank(ctx, 2, 1), DemodBank(other, 2, 1)
    try:
        K.check_refusals(ctx, bank, other_bank)
    finally:
        bank.close(); other_bank.close(); other.close()


# ----------------------------------------------------------------------------------------------- behind a pipeline
FS, M, BLOCK, CENTER, NB, NEXEC = 2400000, 4, 40000, 100000000, 6, 4
KINDS = [("NBFM", 12500), ("AM", 6000), ("USB", 5400), ("I/Q", 48000), ("FMS", 200000), ("QPSK", 200000), ("NBFM", 12500), ("NBFM", 12500), ("HOST", 12500)]
GATED, QPSK_SLOT, OFF_SLOT, SKIP_SLOT, HOST_SLOT, MUTED_SLOT = (0, 1, 2, 3, 4), 5, 6, 7, 8, 2
RECORD = {0: H.CSDR_RECORD_SILENCE, 1: H.CSDR_RECORD_SKIP_SILENCE, 2: H.CSDR_RECORD_ALWAYS, 3: H.CSDR_RECORD_SILENCE, 4: H.CSDR_RECORD_SKIP_SILENCE}
FRAMES = 800


def _iq():
    freqs = demod_frequencies(CENTER, FS, 7) + [CENTER + 1700000, 0]          # slot 7: 500 kHz from the nearest centre, beyond the shift bound of 450 kHz
    freqs[HOST_SLOT] = freqs[0] + 20000
    sig = ["NBFM", "AM", "USB", "NBFM", "FMS", "NBFM", "NBFM"]
    x = synth_iq(NEXEC * NB * BLOCK, FS, CENTER, list(zip(sig, freqs[:7])), seed=91)
    env = np.repeat(np.where((np.arange(NEXEC * NB) // 6) % 2 == 0, 1.0, 0.05).astype(np.float32), BLOCK)       # loud and quiet stretches of six blocks
    return freqs, x * env


class _Pipeline:
    def __init__(self, ctx, freqs, x):
        from cubicsdr_amd.engine import DemodBank, SDRPost, SquelchBank
        self.x = x
        self.post = SDRPost(ctx, FS, M, BLOCK, NB)
        self.bank = DemodBank(ctx, len(KINDS), NB)
        for i, ((k, bw), f) in enumerate(zip(KINDS, freqs)):
            if k == "QPSK":
                self.bank.configure_digital(i, self.post, k, bw, f)
            else:
                self.bank.configure(i, self.post, k, bw, f)
        self.bank.set_active(OFF_SLOT, False)
        self.sq = SquelchBank(ctx, 12, NB)                # (more slots than the bank has: the bank's count bounds the walk)

    def execute(self, e):
        self.post.execute(self.x[e * NB * BLOCK:(e + 1) * NB * BLOCK], NB, BLOCK, CENTER)
        self.bank.execute(self.post)

    def close(self):
        for o in (self.sq, self.bank, self.post):
            o.close()


def _thresholds(levels):
    """per gated slot: the threshold, among the quantiles of the checker's level after its first rise, that makes the squelch flip most often while
    keeping every block's level MARGIN_DB away (signalLevel does not depend on the squelch settings, so the ungated trajectory is the gated one)"""
    out = {}
    for s, lv in levels.items():
        lv = np.asarray(lv, np.float64)
        best = None
        for q in np.linspace(0.2, 0.8, 25):
            t = float(np.float32(np.quantile(lv[NB:], q)))
            if np.min(np.abs(lv - t)) < 4 * K.MARGIN_DB:
                continue
            flips = int(np.count_nonzero(np.diff((lv < t).astype(np.int8))))
            if best is None or flips > best[0]:
                best = (flips, t)
        assert best is not None, s
        out[s] = best[1]
    return out


@pytest.fixture(scope="module")
def pipeline(ctx):
    """Pass 1: the four executes alone; the checker, ungated, over the bank's own sums gives every gated slot's level trajectory and from it the
    thresholds.  Pass 2, on a fresh pipeline fed the same samples: process_bank behind every execute, with everything fetched; two mixers."""
    from cubicsdr_amd.engine import AudioMixer
    freqs, x = _iq()
    p = _Pipeline(ctx, freqs, x)
    levels = {s: [] for s in GATED}
    try:
        refs = {s: RefLevelSquelch() for s in GATED}
        for e in range(NEXEC):
            p.execute(e)
            for s in GATED:
                for r in p.bank.results(s):
                    refs[s].step(r.n_audio > 0, r.level_accum, r.level_count, float(r.n_iq) / float(KINDS[s][1]), False, 0.0)
                    levels[s].append(float(refs[s].level))
    finally:
        p.close()
    thr = _thresholds(levels)
    p = _Pipeline(ctx, freqs, x)
    ma, mb = AudioMixer(ctx, len(GATED), 48000, 1 << 17), AudioMixer(ctx, len(GATED), 48000, 1 << 17)
    rec = dict(thr=thr, want=[], items=[], blocks=[], state=[], flags=[], record=[], pcm=[], results=[], mix=[], queued=[])
    try:
        for s in GATED:
            p.sq.set_slot(s, True, thr[s], s == MUTED_SLOT, RECORD[s])
        p.sq.set_slot(QPSK_SLOT, True, -10.0)
        for s in (OFF_SLOT, SKIP_SLOT, HOST_SLOT):
            p.sq.set_slot(s, True, -50.0)
        refs = {s: RefLevelSquelch() for s in GATED + (QPSK_SLOT,)}
        for e in range(NEXEC):
            p.execute(e)
            p.sq.process_bank(p.bank)
            results = {s: p.bank.results(s) for s in range(len(KINDS))}
            want = {}
            for s in GATED + (QPSK_SLOT,):
                en, lv, muted = True, (thr[s] if s in GATED else -10.0), s == MUTED_SLOT
                rows = []
                for r in results[s]:
                    sq = refs[s].step(r.n_audio > 0, r.level_accum, r.level_count, float(r.n_iq) / float(KINDS[s][1]), en, lv)
                    assert abs(float(refs[s].level) - float(np.float32(lv))) >= K.MARGIN_DB, (e, s, refs[s].level, lv)
                    rows.append((refs[s].level, refs[s].floor, refs[s].ceil, (1 if sq else 0) | (2 if refs[s].squelch_break else 0) | (4 if not sq and not muted else 0)))
                want[s] = rows
            rec["want"].append(want)
            rec["results"].append(results)
            rec["blocks"].append([p.sq.blocks(s) for s in range(12)])
            rec["items"].append({s: p.sq.fetch(s) for s in range(12)})
            rec["state"].append({s: p.sq.state(s) for s in range(12)})
            rec["flags"].append(p.sq.flags())
            rec["record"].append(p.sq.record())
            rec["pcm"].append({s: p.bank.pcm16(s) for s in GATED})
            # the gated mixer feed, and the same open blocks pushed one by one from the fetched audio into a second mixer
            ma.push_bank_squelched(p.bank, p.sq, list(GATED))
            n_open = {}
            for s in GATED:
                audio = p.bank.audio(s)
                ch = 2 if KINDS[s][0] in ("I/Q", "FMS") else 1
                n_open[s] = 0
                for r, it in zip(results[s], rec["items"][-1][s]):
                    if it["flags"] & H.CSDR_SQUELCH_OPEN:
                        assert mb.push(s, audio[r.audio_offset:r.audio_offset + r.n_audio], ch, 48000, r.audio_peak)
                        n_open[s] += 1
            rec["queued"].append(([ma.queued(s) for s in GATED], [mb.queued(s) for s in GATED], [n_open[s] for s in GATED]))
            rec["mix"].append((ma.render(FRAMES, NB), mb.render(FRAMES, NB)))
        yield rec
    finally:
        ma.close(); mb.close()
        p.close()


def test_process_bank_against_the_checker(pipeline):
    """NBFM (level from the IQ), AM and USB (from the audio), I/Q and FM stereo (two floats per sample): items against the checker fed the bank's
    own sums -- flags exact, trackers at one ulp; every gated slot opens and closes at least twice; the meters are the last item"""
    for s in GATED:
        sq = np.array([row[3] & 1 for want in pipeline["want"] for row in want[s]])
        assert np.count_nonzero(np.diff(sq)) >= 2, (s, sq, pipeline["thr"][s])
    for e in range(NEXEC):
        for s in GATED + (QPSK_SLOT,):
            want, it = pipeline["want"][e][s], pipeline["items"][e][s]
            assert pipeline["blocks"][e][s] == NB == it.size == len(want), (e, s)
            assert [int(f) for f in it["flags"]] == [w[3] for w in want], (e, s)
            assert np.array_equal(pipeline["flags"][e][s], it["flags"].astype(np.uint8)), (e, s)
            K.same_trackers(np.stack([it["level"], it["floor"], it["ceil"]], 1), [w[:3] for w in want], False, (e, s))
            st = pipeline["state"][e][s]
            assert st[:3] == (it["level"][-1], it["floor"][-1], it["ceil"][-1]) and st[3] == bool(it["flags"][-1] & 2), (e, s)


def test_digital_slot_climbs_without_a_level(pipeline):
    """the QPSK slot produces no audio: have_level is false on every block, signalLevel climbs towards 0 dB, floor and ceiling stay"""
    lv = np.concatenate([pipeline["items"][e][QPSK_SLOT]["level"] for e in range(NEXEC)])
    assert lv.size == NEXEC * NB and np.all(np.diff(lv) > 0) and lv[0] == np.float32(-50.0) and -1e-3 < lv[-1] < 0
    for e in range(NEXEC):
        assert all(r.n_audio == 0 for r in pipeline["results"][e][QPSK_SLOT])
        it = pipeline["items"][e][QPSK_SLOT]
        assert np.all(it["floor"] == np.float32(-30)) and np.all(it["ceil"] == np.float32(30))
    assert pipeline["items"][-1][QPSK_SLOT]["flags"][-1] == 6                                  # above -10 dB: open, squelchBreak


def test_unstepped_slots_keep_their_state(pipeline):
    """the inactive slot, the slot tuned beyond the shift bound and the CSDR_MODEM_HOST slot report 0 blocks and stay as constructed"""
    fresh = (np.float32(-100), np.float32(-30), np.float32(30), False)
    for e in range(NEXEC):
        assert pipeline["results"][e][OFF_SLOT] == [] and all(r.skipped for r in pipeline["results"][e][SKIP_SLOT]) and len(pipeline["results"][e][SKIP_SLOT]) == NB
        assert len(pipeline["results"][e][HOST_SLOT]) == NB and not pipeline["results"][e][HOST_SLOT][0].skipped
        for s in (OFF_SLOT, SKIP_SLOT, HOST_SLOT, 9, 10, 11):
            assert pipeline["blocks"][e][s] == 0 and pipeline["items"][e][s].size == 0 and pipeline["state"][e][s] == fresh, (e, s)
            assert not pipeline["flags"][e][s].any()


def test_gated_mix_equals_block_by_block_pushes(pipeline):
    """push_bank_squelched + render against a second mixer fed the same open blocks one by one with csdr_mix_push from csdr_bank_fetch_audio: float
    for float; csdr_mix_queued is the count of open blocks; the muted slot contributes nothing but still records"""
    total_open = 0
    for e in range(NEXEC):
        qa, qb, n_open = pipeline["queued"][e]
        a, b = pipeline["mix"][e]
        assert a.tobytes() == b.tobytes(), e
        assert n_open[GATED.index(MUTED_SLOT)] == 0
        total_open += sum(n_open)
    # the queues drain alike, so after every push they hold the same counts; the first execute's are exactly the open blocks
    assert all(pipeline["queued"][e][0] == pipeline["queued"][e][1] for e in range(NEXEC))
    assert pipeline["queued"][0][0] == pipeline["queued"][0][2]
    assert total_open > 0 and any(np.any(pipeline["mix"][e][0] != 0) for e in range(NEXEC))
    pcm, offs = pipeline["record"][-1]
    assert offs[MUTED_SLOT + 1] - offs[MUTED_SLOT] == pipeline["pcm"][-1][MUTED_SLOT].size > 0


def test_recorder_is_fetch_pcm16_cut_by_the_flags(pipeline):
    """every slot's stretch of csdr_squelch_record equals csdr_bank_fetch_pcm16's samples kept, zeroed or left out block by block by the checker's
    flags and the slot's option"""
    kinds = set()
    for e in range(NEXEC):
        pcm, offs = pipeline["record"][e]
        assert offs[0] == 0 and offs[-1] == pcm.size
        for s in range(12):
            got = pcm[offs[s]:offs[s + 1]]
            if s not in GATED:
                assert got.size == 0, (e, s)
                continue
            full, parts = pipeline["pcm"][e][s], []
            for r, w in zip(pipeline["results"][e][s], pipeline["want"][e][s]):
                blk = full[r.audio_offset:r.audio_offset + r.n_audio]
                squelched = bool(w[3] & 1)
                kinds.add((RECORD[s], squelched))
                if squelched and RECORD[s] == H.CSDR_RECORD_SKIP_SILENCE:
                    continue
                parts.append(np.zeros_like(blk) if squelched and RECORD[s] == H.CSDR_RECORD_SILENCE else blk)
            want = np.concatenate(parts) if parts else np.zeros(0, np.int16)
            assert got.tobytes() == want.tobytes(), (e, s)
    assert kinds == {(o, q) for o in range(3) for q in (False, True)}


def test_the_next_execute_waits_for_the_squelch_bank(ctx, pipeline):
    """the same pipeline again with execute e + 1 issued straight behind process_bank of execute e -- no synchronise between -- and batch e's items,
    flags and recorder stream fetched only then: nothing was rewritten under the reader.  With the bank one execute ahead, the gated push is
    refused (CSDR_ESTATE): the squelch bank's flags belong to a stale execute"""
    from cubicsdr_amd.engine import AudioMixer
    freqs, x = _iq()
    p = _Pipeline(ctx, freqs, x)
    mix = AudioMixer(ctx, len(GATED), 48000, 1 << 17)
    try:
        for s in GATED:
            p.sq.set_slot(s, True, pipeline["thr"][s], s == MUTED_SLOT, RECORD[s])
        p.sq.set_slot(QPSK_SLOT, True, -10.0)
        p.execute(0)
        for e in range(NEXEC):
            p.sq.process_bank(p.bank)
            if e + 1 < NEXEC:
                p.execute(e + 1)
                sl = np.array(GATED, np.int32)
                rc = H.lib().csdr_mix_push_squelched(mix.h, p.bank.h, p.sq.h, sl.ctypes.data, sl.ctypes.data, sl.size)
                assert rc == -4, (e, rc)
                assert [mix.queued(i) for i in range(len(GATED))] == [0] * len(GATED)
            for s in range(12):
                assert p.sq.fetch(s).tobytes() == pipeline["items"][e][s].tobytes(), (e, s)
            assert np.array_equal(p.sq.flags(), pipeline["flags"][e]), e
            pcm, offs = p.sq.record()
            assert np.array_equal(offs, pipeline["record"][e][1]) and pcm.tobytes() == pipeline["record"][e][0].tobytes(), e
    finally:
        mix.close()
        p.close()


# ----------------------------------------------------------------------------------------------- at size
def test_256_slots_128_blocks_at_size(ctx):
    """256 slots x 128 blocks through the explicit form in two processes, synthetic sums, every item against the checker"""
    from cubicsdr_amd.engine import SQUELCH_BLOCK, SquelchBank
    S, B = 256, 128
    rng = np.random.default_rng(5)
    sb = SquelchBank(ctx, S, B)
    refs = [RefLevelSquelch() for _ in range(S)]
    try:
        # the sums of both processes first; a slot's threshold is then the first of a ladder that keeps every block's level MARGIN_DB away
        # (signalLevel does not depend on the squelch settings: its recurrence alone, in the checker's arithmetic, gives the trajectory)
        all_blocks, thr = [], []
        for s in range(S):
            g = np.arange(2 * B)
            loud = ((g + 3 * s) // 20) % 2 == 0
            amp = np.where(loud, 0.1, 2e-4) * (1.0 + 0.004 * rng.random(2 * B))
            blocks = np.zeros(2 * B, SQUELCH_BLOCK)
            blocks["level_count"], blocks["n_in"], blocks["n_audio"] = 208 + (g % 3), 208 + (g % 3), 800
            blocks["level_accum"] = amp * blocks["level_count"]
            all_blocks.append(blocks)
            lvl, traj = float(np.float32(-100.0)), np.zeros(2 * B)
            for b in range(2 * B):
                cur = RefLevelSquelch.linear_to_db(float(blocks["level_accum"][b]) / float(blocks["level_count"][b]))
                st = float(blocks["n_in"][b]) / 12500.0
                lvl = float(np.float32(lvl + (cur - lvl) * 0.5 if cur > lvl else lvl + (cur - lvl) * 0.05 * st * 30.0))
                traj[b] = lvl
            t = next(t for t in (float(np.float32(-30.3 - 0.01 * s - 0.137 * k)) for k in range(40)) if np.min(np.abs(traj - t)) >= 4 * K.MARGIN_DB)
            thr.append(t)
            sb.set_slot(s, True, t, False)
        for call in range(2):
            ins, want_t, want_f = [], np.zeros((S, B, 3), np.float32), np.zeros((S, B), np.uint8)
            for s in range(S):
                blocks = all_blocks[s][call * B:(call + 1) * B]
                lv = thr[s]
                for b in range(B):
                    sq = refs[s].step(True, float(blocks["level_accum"][b]), int(blocks["level_count"][b]), float(blocks["n_in"][b]) / 12500.0, True, lv)
                    assert abs(float(refs[s].level) - lv) >= K.MARGIN_DB, (s, call, b)
                    want_t[s, b] = (refs[s].level, refs[s].floor, refs[s].ceil)
                    want_f[s, b] = (1 if sq else 0) | (2 if refs[s].squelch_break else 0) | (0 if sq else 4)
                ins.append(dict(slot=s, sample_rate=12500, blocks=blocks))
            sb.process(ins)
            flags = sb.flags()
            assert np.array_equal(flags, want_f), (call, np.argwhere(flags != want_f)[:4])
            assert (want_f & 1).any() and not (want_f & 1).all()
            for s in range(S):
                it = sb.fetch(s)
                assert it.size == B and np.array_equal(it["flags"], want_f[s]), (call, s)
                K.same_trackers(np.stack([it["level"], it["floor"], it["ceil"]], 1), want_t[s], False, (call, s))
    finally:
        sb.close()
