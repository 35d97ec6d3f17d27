"""The squelch bank (csdr_squelch: squelch_scan / squelch_pack / squelch_pcm16 of kernels_squelch.hpp, include/csdr_hip.h "Squelch bank"): the cases
that the emulation (tests/test_squelch_emu.py) and the device (tests/test_gpu_squelch.py) share, through the explicit-input form.

The yardstick is oracle.cubicsdr_chain.RefLevelSquelch, one per slot, which tests/test_oracle_pin.py pins bit for bit to the reference's own
DemodulatorThread.cpp; where that thread itself is built (oracle.ref_modems.demodthread_available) one sequence runs against it directly.  Flags
and squelchBreak are exact.  The trackers are bit-identical on the emulation (both sides use the host's log10) and within one float32 ulp on the
device: its double log10 differs from the host's by a few double ulps (about 1e-14 dB), every update is a convex combination stored to float, so
the two sides differ by at most one rounding boundary per step, and an existing one-ulp difference contracts instead of growing.  The recorder's
bytes equal AudioFileWAV's rule restated in numpy over the checker's flags."""
import functools

import numpy as np

import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import SQUELCH_BLOCK, SquelchBank
from oracle.cubicsdr_chain import RefLevelSquelch

SHAPES = (5, 7)                       # slots: the workgroup of four slots has a tail of one and of three
CALLS = (1, 63, 64, 65, 70)           # blocks per slot and process: the 64-lane chunk boundary from both sides, state carried over five processes
MAX_BLOCKS = 70
RATE, N_IN = 48000, 800               # sampleTime = 1/60 s
ABSENT = (4, 2)                       # (slot, process): not named in that process -- its state is kept, it reports 0 blocks
RESET = (4, 3)                        # (slot, process): reset_slot in front of that process
MARGIN_DB = 1e-3                      # the checker's |level - threshold| wherever the squelch is on


def pcm16_of(audio, peak):
    """AudioFileWAV::writePayloadToFileStream's conversion of one AudioThreadInput (src/audio/AudioFileWAV.cpp:133-157), in float32"""
    pk = np.float32(peak)
    scale = np.float32(32767.0) if pk < np.float32(1.0) else np.float32(32767.0) / pk
    return (np.asarray(audio, np.float32) * scale).astype(np.int32).astype(np.int16)


def settings_of(slot, call):
    """(enabled, level_db, muted, record) in force for `slot` during process `call`: constant within a process"""
    if slot == 0:                     # gated from the start; the threshold moves between processes
        return True, (-23.7, -23.7, -26.45, -22.3, -25.1)[call], False, H.CSDR_RECORD_SILENCE
    if slot == 1:                     # gated, muted during two processes; the recorder leaves squelched blocks out
        return True, -25.1, call in (2, 3), H.CSDR_RECORD_SKIP_SILENCE
    if slot == 2:                     # gated; the recorder ignores the squelch
        return True, -23.7, False, H.CSDR_RECORD_ALWAYS
    if slot == 3:                     # the squelch is switched on in front of the third process
        return call >= 2, -27.8, False, H.CSDR_RECORD_SILENCE
    if slot == 4:                     # absent once, reset once
        return True, -26.45, call == 4, H.CSDR_RECORD_SKIP_SILENCE
    if slot == 5:                     # no audio handed over: the level step runs, nothing is recorded
        return True, -22.3, False, H.CSDR_RECORD_SILENCE
    return True, -10.0, False, H.CSDR_RECORD_ALWAYS      # slot 6: never produces audio (a digital slot): the level climbs towards 0 dB and opens


@functools.lru_cache(maxsize=None)
def scenario(n_slots):
    """-> per process: [dict(slot, blocks, audio, settings, want)] with want = the checker's items, flags and state after the process, and the
    recorder's expected stream; computed once and shared (treat as read-only)"""
    refs = [RefLevelSquelch() for _ in range(n_slots)]
    rng = np.random.default_rng(4100 + n_slots)
    flips = [0] * n_slots
    last_sq = [None] * n_slots
    out, g0 = [], 0
    for call, nb in enumerate(CALLS):
        per = []
        for s in range(n_slots):
            if (s, call) == RESET:
                refs[s] = RefLevelSquelch()
            if (s, call) == ABSENT:
                per.append(None)
                continue
            en, lv, muted, rec = settings_of(s, call)
            blocks = np.zeros(nb, SQUELCH_BLOCK)
            chunks, items, flags = [], np.zeros((nb, 3), np.float32), np.zeros(nb, np.uint8)
            for b in range(nb):
                g = g0 + b
                loud = ((g + 5 * s) // 16) % 2 == 0
                amp = (0.1 if loud else 1e-4) * (1.0 + 0.005 * rng.random())
                n_audio = 0 if (s == 6 or (s == 3 and g % 29 == 3)) else 100 + (7 * g + 13 * s) % 57
                if s == 2 and g == 40:
                    n_audio = 5000                                       # more than one pass of the conversion's grid
                count = n_audio if s % 2 else N_IN + (g % 3)             # level from the audio, or from the IQ
                accum = amp * count
                if n_audio and ((s == 3 and g in (20, 150)) or (s == 0 and g == 100)):
                    accum = 0.0                                          # an all-zero block: the 1e-20 clamp
                a = ((12.0 if s == 2 else 1.0) * amp * 5.0 * rng.standard_normal(n_audio)).astype(np.float32)      # slot 2: peaks above 1
                peak = np.float32(np.max(np.abs(a))) if n_audio else np.float32(0)
                blocks[b] = (accum, count if n_audio else 0, N_IN + (g % 3), n_audio, peak)
                sq = refs[s].step(n_audio > 0, accum, count, float(N_IN + (g % 3)) / float(RATE), en, lv)
                if en:
                    assert abs(float(refs[s].level) - float(np.float32(lv))) >= MARGIN_DB, (s, g, refs[s].level, lv)
                    if last_sq[s] is not None and last_sq[s] != sq:
                        flips[s] += 1
                    last_sq[s] = sq
                items[b] = (refs[s].level, refs[s].floor, refs[s].ceil)
                flags[b] = (1 if sq else 0) | (2 if refs[s].squelch_break else 0) | (4 if not sq and not muted else 0)
                chunks.append((a, peak, sq))
            audio = None if s == 5 else (np.concatenate([c[0] for c in chunks]) if chunks else np.zeros(0, np.float32))
            pcm = []
            if audio is not None:
                for a, peak, sq in chunks:
                    if not a.size or (sq and rec == H.CSDR_RECORD_SKIP_SILENCE):
                        continue
                    pcm.append(np.zeros(a.size, np.int16) if (sq and rec == H.CSDR_RECORD_SILENCE) else pcm16_of(a, peak))
            per.append(dict(slot=s, blocks=blocks, audio=audio, settings=(en, lv, muted, rec), items=items, flags=flags,
                            state=(refs[s].level, refs[s].floor, refs[s].ceil, refs[s].squelch_break),
                            pcm=np.concatenate(pcm) if pcm else np.zeros(0, np.int16)))
        out.append(per)
        g0 += nb
    # the precondition, on the checker's own run: every gated slot's squelch flips at least twice
    for s in range(min(n_slots, 6)):
        assert flips[s] >= 2, (s, flips)
    return out


def ulp_apart(a, b):
    """|a - b| in units of the float32 spacing at the larger magnitude"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def same_trackers(got, want, exact, where):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if exact:
        assert got.tobytes() == want.tobytes(), where
    else:
        worst = float(np.max(ulp_apart(got, want))) if got.size else 0.0
        assert worst <= 1.0, (where, worst)


def check_scenario(ctx, n_slots, exact):
    """the whole sequence on one SquelchBank: items, flags, fetch_flags, the meters and the recorder after every process -> blocks checked"""
    sc = scenario(n_slots)
    sb = SquelchBank(ctx, n_slots, MAX_BLOCKS)
    n_checked = 0
    try:
        held = {s: (np.float32(-100), np.float32(-30), np.float32(30), False) for s in range(n_slots)}        # the constructor's values
        for call, per in enumerate(sc):
            if RESET[1] == call and RESET[0] < n_slots:
                sb.reset_slot(RESET[0])
                held[RESET[0]] = (np.float32(-100), np.float32(-30), np.float32(30), False)
                assert sb.state(RESET[0]) == held[RESET[0]]
            inputs = []
            for x in reversed([x for x in per if x is not None]):          # (the order of the inputs is not the order of the recorder's stream)
                sb.set_slot(x["slot"], *x["settings"])
                inputs.append(dict(slot=x["slot"], sample_rate=RATE, blocks=x["blocks"], audio=x["audio"]))
            sb.process(inputs)
            all_flags = sb.flags()
            pcm, offs = sb.record()
            assert offs[0] == 0 and offs[-1] == pcm.size
            for s in range(n_slots):
                x = per[s]
                if x is None:
                    assert sb.blocks(s) == 0 and sb.fetch(s).size == 0 and not all_flags[s].any(), (call, s)
                    assert offs[s + 1] == offs[s]
                    got = sb.state(s)
                    same_trackers(got[:3], held[s][:3], True, (call, s, "kept state"))
                    assert got[3] == held[s][3]
                    continue
                nb = x["blocks"].size
                it = sb.fetch(s)
                assert sb.blocks(s) == nb == it.size, (call, s)
                assert np.array_equal(it["flags"], x["flags"]), (call, s, np.flatnonzero(it["flags"] != x["flags"]))
                assert np.array_equal(all_flags[s, :nb], x["flags"]) and not all_flags[s, nb:].any(), (call, s)
                same_trackers(np.stack([it["level"], it["floor"], it["ceil"]], 1), x["items"], exact, (call, s))
                got = sb.state(s)
                same_trackers(got[:3], (it["level"][-1], it["floor"][-1], it["ceil"][-1]), True, (call, s, "state is the last item"))
                assert got[3] == x["state"][3] == bool(x["flags"][-1] & 2), (call, s)
                held[s] = got
                want = x["pcm"]
                assert offs[s + 1] - offs[s] == want.size, (call, s, offs[s + 1] - offs[s], want.size)
                assert pcm[offs[s]:offs[s + 1]].tobytes() == want.tobytes(), (call, s, "recorder")
                n_checked += nb
        # every record option met squelched and open blocks with audio
        assert any(x is not None and (x["flags"] & 1).any() and not (x["flags"] & 1).all() for per in sc for x in per[:3])
    finally:
        sb.close()
    return n_checked


def check_against_demodthread(ctx, exact):
    """one sequence against the reference's own DemodulatorThread on its thread (the caller has checked demodthread_available): trackers,
    squelchBreak, and `pushed`, which is flag bit 2"""
    import oracle.ref_modems as RM
    rng = np.random.default_rng(23)
    ref = RM.RefDemodThreadCpp(False, 12500, 48000)
    sb = SquelchBank(ctx, 1, 64)
    n, g = 0, 0
    try:
        for call, nb in enumerate((1, 63, 64, 40)):
            en, lv, muted = call >= 1, (-30.0, -30.0, -12.0, -30.0)[call], call == 3
            ref.set(en, lv, muted)
            sb.set_slot(0, en, lv, muted)
            blocks, want = np.zeros(nb, SQUELCH_BLOCK), []
            for b in range(nb):
                n_iq = 208 + g % 3
                amp = 0.25 if (g // 20) % 2 == 1 else 0.003
                iq = (amp * (rng.standard_normal(n_iq) + 1j * rng.standard_normal(n_iq))).astype(np.complex64)
                n_audio = 0 if g % 23 == 7 else 160 + g % 2
                audio = (amp * rng.standard_normal(n_audio)).astype(np.float32)
                want.append(ref.block(iq, audio))
                accum = float(np.sum(np.sqrt(iq.real.astype(np.float64) ** 2 + iq.imag.astype(np.float64) ** 2)))
                blocks[b] = (accum, n_iq, n_iq, n_audio, np.float32(np.max(np.abs(audio))) if n_audio else 0.0)
                g += 1
            sb.process([dict(slot=0, sample_rate=12500, blocks=blocks)])
            it = sb.fetch(0)
            same_trackers(np.stack([it["level"], it["floor"], it["ceil"]], 1), [(w["level"], w["floor"], w["ceil"]) for w in want], exact, ("DemodulatorThread", call))
            assert [bool(f & 2) for f in it["flags"]] == [w["squelch_break"] for w in want], call
            assert [bool(f & 4) for f in it["flags"]] == [w["pushed"] for w in want], call
            n += nb
        assert n == 168
    finally:
        sb.close()
        ref.close()
    return n


def check_refusals(ctx, bank=None, other_bank=None):
    """bad capacities, slots out of range, a slot twice, too many blocks, a record option outside 0 .. 2, capacities too small, process_bank
    without an execute (`bank`) and with a bank of another context (`other_bank`): each refused with its code, and none of them changes anything
    -- the process behind them equals the same process on an undisturbed twin, byte for byte"""
    import ctypes as C
    lib = H.lib()
    sc = scenario(5)
    a, t = SquelchBank(ctx, 5, MAX_BLOCKS), SquelchBank(ctx, 5, MAX_BLOCKS)
    n_refused = 0

    def refused(rc, want):
        nonlocal n_refused
        assert rc == want, (rc, want, lib.csdr_last_error())
        n_refused += 1

    def feed(sb, call):
        ins = []
        for x in sc[call]:
            if x is not None:
                sb.set_slot(x["slot"], *x["settings"])
                ins.append(dict(slot=x["slot"], sample_rate=RATE, blocks=x["blocks"], audio=x["audio"]))
        sb.process(ins)
        return ins
    try:
        h = C.c_void_p()
        for slots, blocks in ((0, 8), (4097, 8), (8, 0)):
            refused(lib.csdr_squelch_create(ctx.h, slots, blocks, C.byref(h)), -1)
        for call in (0, 1):
            feed(a, call); feed(t, call)
        good = feed(t, 2)
        x = good[0]
        refused(lib.csdr_squelch_set_slot(a.h, 0, 1, -20.0, 0, 3), -1)
        refused(lib.csdr_squelch_set_slot(a.h, 0, 1, -20.0, 0, -1), -1)
        refused(lib.csdr_squelch_set_slot(a.h, 5, 1, -20.0, 0, 0), -1)
        refused(lib.csdr_squelch_reset_slot(a.h, -1), -1)
        refused(a.try_process(good + [dict(x, slot=5)]), -1)
        refused(a.try_process(good + [dict(x, slot=-1)]), -1)
        refused(a.try_process(good + [dict(x)]), -1)                                                   # the same slot twice
        refused(a.try_process(good[1:] + [dict(x, blocks=np.zeros(MAX_BLOCKS + 1, SQUELCH_BLOCK), audio=None)]), -1)
        if bank is not None:
            refused(lib.csdr_squelch_process_bank(a.h, bank.h), -4)
        if other_bank is not None:
            refused(lib.csdr_squelch_process_bank(a.h, other_bank.h), -1)
        assert [a.blocks(s) for s in range(5)] == [len(p["blocks"]) if p is not None else 0 for p in sc[1]]
        feed(a, 2)
        for s in range(5):
            assert a.fetch(s).tobytes() == t.fetch(s).tobytes() and a.state(s) == t.state(s), s
        pa, oa = a.record()
        pt, ot = t.record()
        assert pa.tobytes() == pt.tobytes() and np.array_equal(oa, ot) and pa.size > 0
        # the outputs' own refusals
        item = (H.SquelchItem * MAX_BLOCKS)()
        n = C.c_int()
        refused(lib.csdr_squelch_fetch(a.h, 0, item, 3, C.byref(n)), -5)
        refused(lib.csdr_squelch_fetch(a.h, 5, item, MAX_BLOCKS, C.byref(n)), -1)
        buf = np.empty(5 * MAX_BLOCKS, np.uint8)
        refused(lib.csdr_squelch_fetch_flags(a.h, buf.ctypes.data_as(C.c_void_p), buf.size - 1), -5)
        pcm, offs = np.empty(pa.size, np.int16), np.empty(6, np.int64)
        refused(lib.csdr_squelch_record(a.h, pcm.ctypes.data_as(C.c_void_p), pa.size - 1, offs.ctypes.data_as(C.c_void_p)), -5)
        assert lib.csdr_squelch_record(a.h, pcm.ctypes.data_as(C.c_void_p), pa.size, offs.ctypes.data_as(C.c_void_p)) == 0 and pcm.tobytes() == pa.tobytes()
        p, stride = a.device_items()
        assert p and stride == MAX_BLOCKS
        assert n_refused == 15 + (bank is not None) + (other_bank is not None)
    finally:
        a.close(); t.close()
