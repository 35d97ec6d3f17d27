"""The scope bank (csdr_scopebank: scopebank_wave / scopebank_spectrum of kernels_scopebank.hpp, include/csdr_hip.h "Scope bank"): the cases that the
emulation (tests/test_scopebank_emu.py) and the device (tests/test_gpu_scopebank.py) share.

Two yardsticks.  The reference's own class, oracle.ref_modems.RefScopeCpp, one per slot, by the rule of tests/test_gpu_io.py::_compare_scope_item:
metadata and x positions equal, waveform items bit for bit, spectrum y values at rel_err < 1e-5, floor and ceiling within 1e-5 |ceil|.  And
csdr_scope itself, byte for byte: every property (a csdr_scope per slot, one frame per call against many, independence of the slots, reset_slot,
the enable switches, a NaN sample, the refusals) is an equality of bytes and never skips."""
import ctypes as C

import numpy as np

import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import ScopeBank, ScopeProcessor
from tests.test_gpu_io import TOL, _compare_scope_item, _need

SIZES = (32, 64, 1024, 4096)          # 32: an odd bit count (lds_fft's radix-2 head); 64: an even one; 1024: DEFAULT_SCOPE_FFT_SIZE; 4096: the limit, LDS above 64 KB
BYTE_SIZES = (4, 32, 64, 1024)        # the byte-for-byte checks; 4 is the smallest size csdr_scope_setup takes
SLOTS, FRAMES = 8, 10
MAX_FRAMES, MAX_SAMPLES = 4, 4096
CALLS = (1, 1, 1, 3, 4)               # frames per slot and call
EMPTY_BEFORE = (3, 7)                 # slot (h): an n = 0 item in front of these frames
OUT_SIZE_A = {32: 4, 64: 8, 1024: 133, 4096: 533}         # floor(L/2 * 12500 / 48000) in float arithmetic (:194-200)
OUT_SIZE_D = {32: 12, 64: 24, 1024: 384, 4096: 1536}      # floor(L/2 * 36000 / 48000)
EMPTY = dict(data=np.zeros(0, np.float32), channels=1, type=0, sample_rate=48000, input_rate=48000)


def _tone(rng, f, a, n, fs=48000.0):
    t = np.arange(n)
    return (a * np.sin(2 * np.pi * f * t / fs) + 0.01 * rng.standard_normal(n)).astype(np.float32)


def make_frames(nan=False):
    """slot -> [[frame dict, ...] per frame index] (the inner list: what is submitted for that index, in order; slot (h) puts an empty item in
    front of two of its frames), or None for the slot that receives nothing.  Tones over 1 % noise, a seed per slot."""
    out = {}
    for s in range(SLOTS):
        rng = np.random.default_rng(1000 + 31 * s)
        fr = []
        for k in range(FRAMES):
            if s in (0, 7):          # (a), (h): mono audio tap labelled below the audio rate
                f = dict(data=_tone(rng, 900 + 130 * k + 40 * s, 0.3 + 0.05 * k, 800 + (k & 1)), channels=1, type=0, sample_rate=12500, input_rate=48000)
            elif s == 1:             # (b): shorter than L and than max_scope_samples, peak above 1
                f = dict(data=_tone(rng, 700 + 50 * k, 2.5, 90), channels=1, type=0, sample_rate=5400, input_rate=5400)
            elif s == 2:             # (c): more than the scope shows; for L < 2048 more than the transform takes
                f = dict(data=_tone(rng, 3000 + 200 * k, 0.2 + 0.02 * k, 2048), channels=1, type=0, sample_rate=200000, input_rate=200000)
            elif s == 3:             # (d): stereo, planar halves
                f = dict(data=np.concatenate([_tone(rng, 400 + 30 * k, 0.3, 800), _tone(rng, 900 + 70 * k, 0.6, 800)]), channels=2, type=1, sample_rate=36000, input_rate=48000)
            elif s == 4:             # (e): X / Y pairs
                xy = np.empty(1600, np.float32)
                xy[0::2] = _tone(rng, 500 + 20 * k, 0.5, 800); xy[1::2] = _tone(rng, 500 + 20 * k, 0.5, 800)[::-1]
                f = dict(data=xy, channels=2, type=2, sample_rate=48000, input_rate=48000)
            elif s == 5:             # (f): receives nothing
                fr = None
                break
            else:                    # (g): interleaved pairs as a stereo demodulator wrote them, read in place
                ab = np.empty(1600, np.float32)
                ab[0::2] = _tone(rng, 600 + 45 * k, 0.7, 800); ab[1::2] = _tone(rng, 1500 + 25 * k, 0.4, 800)
                f = dict(data=ab, channels=2, type=1, sample_rate=48000, input_rate=48000)
                f.update(dict(layout=1, scale=1.0) if k < FRAMES // 2 else dict(layout=2, scale=0.75))
            fr.append([EMPTY, f] if s == 7 and k in EMPTY_BEFORE else [f])
        out[s] = fr
    if nan:
        v = out[1][4][0]["data"].copy()
        v[37] = np.nan
        out[1][4][0] = dict(out[1][4][0], data=v)
    return out


def as_audio_thread_input(f):
    """the AudioThreadInput::data the reference would have built for a frame read in place (csdr_hip.h, csdr_scope_frame.layout)"""
    d, lay = f["data"], f.get("layout", 0)
    if lay == 0:
        return d
    sc = np.float32(f["scale"])
    a, b = d[0::2] * sc, d[1::2] * sc
    return np.concatenate([a, b] if lay == 1 else [b, a]).astype(np.float32)


def call_plan(frames, calls=CALLS, order="slot", only=None):
    """[[(slot, frame dict)]] per call: `calls[k]` frame indices of every fed slot; order "slot": slot by slot, "item": index by index with the slots
    reversed (the interleavings the independence property compares); only: feed just these slots"""
    fed = [s for s in sorted(frames) if frames[s] is not None and (only is None or s in only)]
    plan, at = [], 0
    for per in calls:
        if order == "slot":
            plan.append([(s, f) for s in fed for k in range(at, at + per) for f in frames[s][k]])
        else:
            plan.append([(s, f) for k in range(at, at + per) for s in reversed(fed) for f in frames[s][k]])
        at += per
    return plan


def items_of(sb):
    """{slot: [(waveform item or None, spectrum item or None)]} of the last call"""
    return {s: [(sb.fetch(s, j, False), sb.fetch(s, j, True)) for j in range(sb.frames(s))] for s in range(sb.max_slots)}


def run_plan(sb, plan, before_call=None):
    got = {s: [] for s in range(sb.max_slots)}
    for k, call in enumerate(plan):
        if before_call:
            before_call(k)
        sb.process(call)
        for s, it in items_of(sb).items():
            got[s] += it
    return got


def same_item(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a["points"].tobytes() != b["points"].tobytes():
        return False
    for k in ("mode", "spectrum", "channels", "input_rate", "sample_rate", "fft_size"):
        if a[k] != b[k]:
            return False
    return all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in ("fft_floor", "fft_ceil"))


def same_bytes(a, b):
    """two lists of (waveform, spectrum) pairs hold identical bytes"""
    return len(a) == len(b) and all(same_item(x[0], y[0]) and same_item(x[1], y[1]) for x, y in zip(a, b))


def scope_per_slot(ctx, L, plan, before_call=None):
    """the yardstick that never skips: one csdr_scope per fed slot, given the slot's non-empty frames of every call -> {slot: [(wave, spectrum)]}"""
    scopes, got = {}, {s: [] for s in range(SLOTS)}
    try:
        for k, call in enumerate(plan):
            if before_call:
                before_call(k, scopes)
            for s in sorted({s for s, _ in call}):
                batch = [f for t, f in call if t == s and f["data"].size]
                if not batch:
                    continue
                if s not in scopes:
                    scopes[s] = ScopeProcessor(ctx, L, max_frames=MAX_FRAMES, max_samples=MAX_SAMPLES)
                scopes[s].process(batch)
                got[s] += [(scopes[s].fetch(j, False), scopes[s].fetch(j, True)) for j in range(len(batch))]
    finally:
        for sp in scopes.values():
            sp.close()
    return got


def check_against_reference(ctx, L):
    """every produced item of every slot against its RefScopeCpp; returns (items checked, worst spectrum error)"""
    import oracle.ref_modems as RM
    _need(RM.scope_available(), "libref_scope.so")
    frames = make_frames()
    refs = {s: RM.RefScopeCpp(L) for s in range(SLOTS) if frames[s] is not None}
    sb = ScopeBank(ctx, L, SLOTS, MAX_FRAMES, MAX_SAMPLES)
    n, worst = 0, 0.0
    try:
        got = run_plan(sb, call_plan(frames))
        for s in range(SLOTS):
            if frames[s] is None:
                assert not got[s], s
                continue
            real = [f for k in range(FRAMES) for f in frames[s][k] if f["data"].size]
            assert len(got[s]) == len(real) == FRAMES, (L, s, len(got[s]))
            for j, (f, (wave, spec)) in enumerate(zip(real, got[s])):
                want = refs[s].push(as_audio_thread_input(f), f["channels"], f["input_rate"], f["sample_rate"], f["type"])
                assert len(want) == 2 and not want[0]["spectrum"] and want[1]["spectrum"], (L, s, j)
                _compare_scope_item(wave, want[0], (L, s, j, "wave"))
                e = _compare_scope_item(spec, want[1], (L, s, j, "spectrum"))
                print("scope bank L = %d slot %d frame %d: spectrum rel_err %.3g" % (L, s, j, e))
                assert e < TOL, (L, s, j, e)
                worst = max(worst, e)
                n += 2
            assert got[s][0][0]["mode"] == (2 if s == 4 else 1 if s in (3, 6) else 0)
        assert got[0][0][1]["points"].size == 2 * OUT_SIZE_A[L] and got[7][0][1]["points"].size == 2 * OUT_SIZE_A[L]
        assert got[3][0][1]["points"].size == 2 * OUT_SIZE_D[L]
        assert got[1][0][0]["points"].size == 2 * 90 and got[2][0][0]["points"].size == 2 * 1024 and got[2][0][1]["points"].size == L
    finally:
        sb.close()
        for r in refs.values():
            r.close()
    return n, worst


def check_properties(ctx, L):
    """bit for bit: a csdr_scope per slot; one frame per call against many; a slot alone against the slot among the others in two interleavings;
    reset_slot; the enable switches; a NaN sample"""
    frames = make_frames()
    fed = [s for s in range(SLOTS) if frames[s] is not None]

    def fresh(max_frames=MAX_FRAMES):
        return ScopeBank(ctx, L, SLOTS, max_frames, MAX_SAMPLES)
    a = fresh()
    many = run_plan(a, call_plan(frames))
    a.close()
    assert [len(many[s]) for s in range(SLOTS)] == [FRAMES if s in fed else 0 for s in range(SLOTS)]
    # every slot against a csdr_scope of its own
    scope = scope_per_slot(ctx, L, call_plan(frames))
    for s in range(SLOTS):
        assert same_bytes(many[s], scope[s]), (L, s, "csdr_scope")
    # one frame per call, and the other interleaving with every frame in one call
    b = fresh(1)
    single = run_plan(b, call_plan(frames, (1,) * FRAMES))
    b.close()
    c = fresh(FRAMES)
    inter = run_plan(c, call_plan(frames, (FRAMES,), order="item"))
    c.close()
    for s in range(SLOTS):
        assert same_bytes(many[s], single[s]), (L, s, "one frame per call")
        assert same_bytes(many[s], inter[s]), (L, s, "interleaving")
    for s in (0, 3, 7):
        d = fresh()
        got = run_plan(d, call_plan(frames, only=(s,)))
        d.close()
        assert same_bytes(many[s], got[s]), (L, s, "alone")
        assert all(not got[k] for k in range(SLOTS) if k != s)
    # reset_slot: slot 3 starts over with its own frames 0 .. 3 while the others go on with 4 .. 7
    e = fresh()
    first = run_plan(e, call_plan(frames, (4,)))
    e.reset_slot(3)
    e.process([(s, f) for s in fed for k in range(4, 8) for f in frames[s][k - 4 if s == 3 else k]])
    second = items_of(e)
    e.close()
    assert same_bytes(first[3], second[3]) and same_bytes(second[3], many[3][:4]), (L, "reset_slot")
    for s in fed:
        if s != 3:
            assert same_bytes(first[s] + second[s], many[s][:8]), (L, s, "neighbour of a reset slot")
    # the enable switches work between calls: spectrum only for call 1, scope only for call 2 (a spectrum that is off advances no averager)
    def switch_bank(sb):
        return lambda k: sb.set_enabled(*{1: (False, True), 2: (True, False)}.get(k, (True, True)))

    def switch_scopes(k, scopes):
        for sp in scopes.values():
            sp.set_enabled(*{1: (False, True), 2: (True, False)}.get(k, (True, True)))
    g = fresh()
    sw = run_plan(g, call_plan(frames), switch_bank(g))
    g.close()
    sw_scope = scope_per_slot(ctx, L, call_plan(frames), switch_scopes)
    for s in fed:
        assert same_bytes(sw[s], sw_scope[s]), (L, s, "enable switches")
        assert sw[s][1][0] is None and sw[s][2][1] is None and sw[s][2][0] is not None, (L, s)
        assert (sw[s][1][1] is None) == (many[s][1][1] is None)
    # one NaN sample in slot (b), frame 4: every other slot's bytes are unchanged, slot (b) shows the NaN mask csdr_scope shows
    bad = make_frames(nan=True)
    h = fresh()
    got = run_plan(h, call_plan(bad))
    h.close()
    nan_scope = scope_per_slot(ctx, L, call_plan(bad, only=(1,)))
    for s in range(SLOTS):
        if s != 1:
            assert same_bytes(got[s], many[s]), (L, s, "neighbour of a NaN")
    assert len(got[1]) == len(nan_scope[1]) == FRAMES
    n_nan = 0
    for j, (x, y) in enumerate(zip(got[1], nan_scope[1])):
        for p, q in zip(x, y):
            assert (p is None) == (q is None), (L, j)
            if p is not None:
                assert np.array_equal(np.isnan(p["points"]), np.isnan(q["points"])), (L, j, "NaN mask")
                assert np.array_equal(p["points"], q["points"], equal_nan=True), (L, j)
                n_nan += int(np.isnan(p["points"]).sum())
    assert n_nan > 0
    assert same_bytes(got[1][:4], many[1][:4])


def check_refusals(ctx, L, bank=None):
    """bad sizes and counts, a slot out of range, three channels, a bad layout, a frame of max_samples + 1 floats, max_frames + 1 frames for one
    slot, process_bank without an execute (`bank`: a demodulator bank that has not executed): each is refused with its code and changes nothing
    -- the calls around it equal the same calls on an undisturbed twin, byte for byte"""
    frames = make_frames()
    lib = H.lib()
    a, t = ScopeBank(ctx, L, SLOTS, MAX_FRAMES, MAX_SAMPLES), ScopeBank(ctx, L, SLOTS, MAX_FRAMES, MAX_SAMPLES)
    good = frames[0][0][0]
    n_refused = 0

    def refused(rc, want):
        nonlocal n_refused
        assert rc == want, (rc, want, H.lib().csdr_last_error())
        assert [a.frames(s) for s in range(SLOTS)] == [t.frames(s) for s in range(SLOTS)]
        n_refused += 1
    try:
        got, twin = {s: [] for s in range(SLOTS)}, {s: [] for s in range(SLOTS)}
        for k, call in enumerate(call_plan(frames)):
            if k == 2:
                for bad_l in (3, 48, 8192, 0):
                    refused(lib.csdr_scopebank_setup(a.h, bad_l, SLOTS, MAX_FRAMES, MAX_SAMPLES), -6)
                for slots, mf, ms in ((0, MAX_FRAMES, MAX_SAMPLES), (4097, MAX_FRAMES, MAX_SAMPLES), (SLOTS, 0, MAX_SAMPLES), (SLOTS, MAX_FRAMES, 0)):
                    refused(lib.csdr_scopebank_setup(a.h, L, slots, mf, ms), -1)
            if k == 3:
                rest = [(s, f) for s, f in call]
                refused(a.try_process(rest + [(SLOTS, good)]), -1)
                refused(a.try_process(rest + [(-1, good)]), -1)
                refused(a.try_process(rest + [(2, dict(good, channels=3))]), -1)
                refused(a.try_process(rest + [(2, dict(good, layout=3))]), -1)
                refused(a.try_process(rest + [(2, dict(good, data=np.zeros(MAX_SAMPLES + 1, np.float32)))]), -5)
                refused(a.try_process([(2, good)] * (MAX_FRAMES + 1)), -5)
                refused(a.try_process(rest + [(0, good)] * 2), -5)              # three frames of the call and two more for slot (a)
            if k == 4 and bank is not None:
                refused(lib.csdr_scopebank_process_bank(a.h, bank.h), -4)
            a.process(call); t.process(call)
            for s, it in items_of(a).items():
                got[s] += it
            for s, it in items_of(t).items():
                twin[s] += it
        for s in range(SLOTS):
            assert same_bytes(got[s], twin[s]), (L, s)
        assert sum(len(v) for v in got.values()) == 7 * FRAMES and n_refused == 15 + (bank is not None)
        # the fetches' own refusals
        buf = np.empty(2 * MAX_SAMPLES, np.float32)
        info = H.ScopeInfo()
        assert lib.csdr_scopebank_fetch(a.h, 2, MAX_FRAMES, 0, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(info)) == -1
        assert lib.csdr_scopebank_fetch(a.h, 5, 0, 0, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(info)) == -1
        assert lib.csdr_scopebank_fetch(a.h, 2, 0, 0, buf.ctypes.data_as(C.c_void_p), 7, C.byref(info)) == -5
        p, n, st = a.device_points(2, True)
        assert p and n == 4 and st == L
        p, n, st = a.device_points(2, False)
        assert p and n == 4 and st == 2 * MAX_SAMPLES
    finally:
        a.close(); t.close()
