"""The spectrum bank (csdr_specbank: specbank_process of kernels_specbank.hpp, include/csdr_hip.h "Spectrum bank") against
oracle.cubicsdr_chain.RefSpectrum, one model per slot, and the cases that the emulation (tests/test_specbank_emu.py), the device
(tests/test_gpu_specbank.py) and the pin against the reference's own class (tests/test_specbank_pin.py) share.

The yardstick is the project's: rel_err(points, want) < TOL = 1e-5 per frame (tests/util.py), ceiling and floor within TOL of the ceiling, the NaN
masks identical.  The properties (one item per call against many, independence of the slots, reset_slot, the refusals) are bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import SpectrumBank
from tests.util import rel_err, synth_iq

TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (16, 32, 256, 2048)           # Fi = 32: an odd bit count (lds_fft's radix-2 head); 64: an even one; 512; 4096: the limit
PEAK_SIZES = (32, 256)
N_ITEMS = 12
CALLS = (1, 1, 1, 3, 6)               # items per slot and call
PEAK_CALLS = (1, 1, 3, 1, 6, 14, 14)  # the setter works between calls: before items 2 and 5; then past the 30-input countdown
SLOTS = 6
# NaN samples, (slot, item, position as a fraction of the item): one in slot (c), whose every input replaces the whole window -- the NaN is gone with
# the next input and the averagers are repaired frame by frame (:494-498: finite points again two frames later) -- and one in slot (a), whose window
# slides by a tenth per input and keeps the sample to the end of the case
NANS = ((2, 3, 0.25), (0, 3, 0.5))
NAN_REPAIR_SLOT, NAN_REPAIR_ITEM = 2, 3


def backend():
    import oracle.liquid_api as A
    if A.available("ref"):
        return "ref"
    if not A.available("port"):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "_ref/liboracle_port.so"], check=True)
    return "port"


def lengths(F, n_items=N_ITEMS):
    """slot -> the lengths of its inputs, as fractions of Fi rounded to integers (None: the slot receives nothing)"""
    Fi = 2 * F
    a = [int(round(0.1 * Fi))] * N_ITEMS
    a[6] = 0                                                                  # (a) prime, then slide; one ignored item
    b = [Fi - 1, 1, Fi, Fi + 7, 3, Fi - 1, 2, Fi, 1, Fi // 2, Fi // 2, 5]     # (b) the boundaries of every branch
    c = [2 * Fi] * N_ITEMS                                                    # (c) never primes
    base = int(round(0.1015 * Fi))
    d = [max(1, base + (-1, 0, 1, 0, 1, -1)[k % 6]) for k in range(N_ITEMS)]  # (d) as msresamp output counts move
    f = [Fi, Fi + 1, 3, 5, Fi, 2, Fi - 1, 1, Fi, 4, 4, 4]                     # (f) FULL first, then the late priming on the first short input
    out = {0: a, 1: b, 2: c, 3: d, 4: None, 5: f}
    if n_items > N_ITEMS:
        out = {s: (None if v is None else [v[k % N_ITEMS] for k in range(n_items)]) for s, v in out.items()}
    return out


def make_inputs(F, n_items=N_ITEMS, nan=True):
    """slot -> [complex64 arrays], cut from one seeded carriers-over-noise stream per slot"""
    data = {}
    for s, ln in lengths(F, n_items).items():
        if ln is None:
            data[s] = None
            continue
        x = synth_iq(sum(ln), 48000.0, 0, [("NBFM", 5000.0 + 700.0 * s), ("AM", -9000.0 + 300.0 * s)], seed=900 + 17 * s + F)
        cut, at = [], 0
        for n in ln:
            cut.append(x[at:at + n].copy())
            at += n
        data[s] = cut
    if nan:
        for slot, item, pos in NANS:
            v = data[slot][item]
            v[int(len(v) * pos)] = np.complex64(complex(np.nan, 0.25))
    return data


class Model:
    """one RefSpectrum per slot, fed as the header's section says: an empty item is no input at all"""

    def __init__(self, F, slots=SLOTS, average_rate=0.65, scale=1.0):
        from oracle.cubicsdr_chain import RefSpectrum
        be = backend()
        self.m = [RefSpectrum(be, F, average_rate, scale) for _ in range(slots)]

    def set_peak_hold(self, on):
        for m in self.m:
            m.set_peak_hold(on)

    def feed(self, slot, x):
        """-> None or (points, ceiling, floor, hold or None)"""
        if x is None or len(x) == 0:
            return None
        return self.m[slot].process_input(x)


def call_plan(data, calls, order="slot"):
    """[[(slot, item index)]] per call: `calls[k]` items of every fed slot; order "slot": slot by slot, "item": item by item with the slots
    reversed (the interleavings the independence property compares)"""
    plan, at = [], 0
    slots = [s for s in sorted(data) if data[s] is not None]
    for per in calls:
        if order == "slot":
            plan.append([(s, k) for s in slots for k in range(at, at + per)])
        else:
            plan.append([(s, k) for k in range(at, at + per) for s in reversed(slots)])
        at += per
    return plan


def run_call(sb, data, call):
    """one process call -> {slot: [(points, ceiling, floor, hold or None)]} of the frames it produced"""
    sb.process([(s, data[s][k]) for s, k in call])
    out = {}
    for s in range(sb.max_slots):
        out[s] = []
        for j in range(sb.frames(s)):
            p, ce, fl = sb.fetch(s, j)
            out[s].append((p, ce, fl, sb.fetch_hold(s, j)))
    return out


def run_plan(sb, data, plan, before_call=None):
    """-> {slot: [frames in order]} over all calls of the plan; before_call(k) runs in front of call k"""
    got = {s: [] for s in range(sb.max_slots)}
    for k, call in enumerate(plan):
        if before_call:
            before_call(k)
        for s, fr in run_call(sb, data, call).items():
            got[s] += fr
    return got


def same_bytes(a, b):
    """two frame lists hold identical bytes"""
    if len(a) != len(b):
        return False
    for (p, ce, fl, h), (q, ce2, fl2, h2) in zip(a, b):
        if p.tobytes() != q.tobytes() or np.float64(ce).tobytes() != np.float64(ce2).tobytes() or np.float64(fl).tobytes() != np.float64(fl2).tobytes():
            return False
        if (h is None) != (h2 is None) or (h is not None and h.tobytes() != h2.tobytes()):
            return False
    return True


def check_frame(got, want, where):
    """the yardstick: one frame of the bank against the model's"""
    pts, ce, fl, hold = got
    wp, wce, wfl, whold = want
    worst = 0.0
    for g, w, what in ((pts, wp, "points"), (hold, whold, "hold")):
        assert (g is None) == (w is None), (where, what)
        if g is None:
            continue
        assert np.array_equal(g[0::2], w[0::2]), (where, what, "x")
        bad = np.isnan(w)
        assert np.array_equal(np.isnan(g), bad), (where, what, int(bad.sum()), int(np.isnan(g).sum()))
        if not bad.all():
            e = rel_err(g[~bad], w[~bad])
            worst = max(worst, e)
            assert e < TOL, (where, what, e)
    for g, w in ((ce, wce), (fl, wfl)):
        assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= TOL * abs(wce), (where, ce, wce, fl, wfl)
    return worst


def model_frames(F, data, n_items, peak_events=None):
    """{slot: [frames]} of the model; peak_events: {item index: on} -> set_peak_hold in front of that item on every slot"""
    m = Model(F)
    want = {s: [] for s in range(SLOTS)}
    for k in range(n_items):
        if peak_events and k in peak_events:
            m.set_peak_hold(peak_events[k])
        for s in range(SLOTS):
            if data[s] is None:
                continue
            w = m.feed(s, data[s][k])
            if w is not None:
                want[s].append(w)
    return want


def check_against_model(ctx, F):
    """the five call sizes, every slot, every frame; returns (frames checked, worst error)"""
    data = make_inputs(F)
    want = model_frames(F, data, N_ITEMS)
    sb = SpectrumBank(ctx, F, SLOTS, max(CALLS))
    try:
        got = run_plan(sb, data, call_plan(data, CALLS))
    finally:
        sb.close()
    n, worst, nan_frames = 0, 0.0, 0
    for s in range(SLOTS):
        assert len(got[s]) == len(want[s]), (F, s, len(got[s]), len(want[s]))
        for j, (g, w) in enumerate(zip(got[s], want[s])):
            worst = max(worst, check_frame(g, w, (F, s, j)))
            nan_frames += int(np.isnan(w[0]).any())
            n += 1
    assert not got[4] and not want[4]                       # the slot that receives nothing
    assert len(want[0]) == N_ITEMS - 2                      # (a): one priming input, one ignored item
    assert len(want[2]) == N_ITEMS                          # (c): a frame per input
    assert len(want[5]) == N_ITEMS - 1                      # (f): the late priming swallows one input
    # slot (c) makes a frame per input.  The NaN input's own frame still shows finite points (the second averager reads the OLD first one, :496), the
    # frame behind it is all NaN, and from the second frame behind it on both averagers have been re-seeded (:495, :497): finite again, within TOL
    # (check_frame compared them above) -- what a kernel without the two repairs, or with them in another order, does not give
    k = NAN_REPAIR_ITEM
    masks = [np.isnan(w[0][1::2]) for w in want[NAN_REPAIR_SLOT]]
    assert not masks[k].any() and masks[k + 1].all() and not any(m.any() for m in masks[k + 2:]), [int(m.sum()) for m in masks]
    for j in range(k + 2, N_ITEMS):
        g = got[NAN_REPAIR_SLOT][j]
        assert np.isfinite(g[0]).all() and np.isfinite(g[1]) and np.isfinite(g[2]), (F, j)
    assert all(np.isnan(w[0][1::2]).all() for w in want[0][k:])      # slot (a) keeps its NaN sample in the window
    assert nan_frames == 1 + len(want[0][k:])
    print("spectrum bank F = %d: %d frames, %d of them with NaN points as in the model, worst rel_err %.3g" % (F, n, nan_frames, worst))
    return n, worst


def check_peak_hold(ctx, F):
    """enabled before item 2, enabled again before item 5 (the 30-input countdown), 40 inputs: hold points and the peak-scaled ceiling / floor"""
    n_items = sum(PEAK_CALLS)
    data = make_inputs(F, n_items, nan=False)
    events = {2: True, 5: True}
    want = model_frames(F, data, n_items, events)
    starts = np.cumsum((0,) + PEAK_CALLS[:-1]).tolist()
    sb = SpectrumBank(ctx, F, SLOTS, max(PEAK_CALLS))
    try:
        assert not sb.get_peak_hold()
        got = run_plan(sb, data, call_plan(data, PEAK_CALLS), lambda k: sb.set_peak_hold(True) if starts[k] in events else None)
        assert sb.get_peak_hold()
    finally:
        sb.close()
    held = 0
    for s in range(SLOTS):
        assert len(got[s]) == len(want[s]), (F, s)
        for j, (g, w) in enumerate(zip(got[s], want[s])):
            check_frame(g, w, (F, s, j))
            held += int(w[3] is not None)
    # slot (c) makes a frame per input: hold on inputs 3, 4 (behind the first reset), then from input 35 on (5 + 30 inputs later)
    assert [j for j, w in enumerate(want[2]) if w[3] is not None] == [3, 4] + list(range(35, n_items))
    # slot (a) skips an empty item: its countdown ends one item later
    assert sum(w[3] is not None for w in want[0]) < sum(w[3] is not None for w in want[3])
    return held


def check_properties(ctx, F):
    """bit for bit: one item per call against many per call; a slot alone against the slot among the others in two interleavings; reset_slot"""
    data = make_inputs(F)
    fed = [s for s in sorted(data) if data[s] is not None]

    def fresh(max_frames=max(CALLS)):
        return SpectrumBank(ctx, F, SLOTS, max_frames)
    a = fresh()
    many = run_plan(a, data, call_plan(data, CALLS))
    a.close()
    b = fresh(1)
    single = run_plan(b, data, call_plan(data, (1,) * N_ITEMS))
    b.close()
    c = fresh(N_ITEMS)
    inter = run_plan(c, data, call_plan(data, (N_ITEMS,), order="item"))
    c.close()
    for s in range(SLOTS):
        assert same_bytes(many[s], single[s]), (F, s, "one item per call")
        assert same_bytes(many[s], inter[s]), (F, s, "interleaving")
    for s in (0, 1, 5):
        alone = {k: (v if k == s else None) for k, v in data.items()}
        d = fresh()
        got = run_plan(d, alone, call_plan(alone, CALLS))
        d.close()
        assert same_bytes(many[s], got[s]), (F, s, "alone")
        assert all(not got[k] for k in range(SLOTS) if k != s)
    # reset_slot: slot 1 starts over with its own inputs 0 .. 5 while the others go on with 6 .. 11
    e = fresh(6)
    first = run_plan(e, data, call_plan(data, (6,)))
    e.reset_slot(1)
    e.process([(s, data[s][k - 6 if s == 1 else k]) for k in range(6, 12) for s in fed])
    second = {s: [(e.fetch(s, j) + (e.fetch_hold(s, j),)) for j in range(e.frames(s))] for s in range(SLOTS)}
    e.close()
    assert same_bytes(second[1], many[1][:len(first[1])]) and same_bytes(first[1], second[1]), (F, "reset_slot")
    for s in fed:
        if s != 1:
            assert same_bytes(first[s] + second[s], many[s]), (F, s, "neighbour of a reset slot")


def check_refusals(ctx, F, bank=None):
    """a bad F, max_frames exceeded, process_bank without an execute (`bank`: a demodulator bank that has not executed): each is refused with its
    code and changes nothing -- the following valid calls equal the same calls on an undisturbed twin"""
    data = make_inputs(F)
    lib = H.lib()
    a, t = SpectrumBank(ctx, F, SLOTS, 3), SpectrumBank(ctx, F, SLOTS, 3)
    try:
        plan = call_plan(data, (1, 1, 1, 3, 3, 3))
        n_bad = 0
        got, twin = {s: [] for s in range(SLOTS)}, {s: [] for s in range(SLOTS)}
        for k, call in enumerate(plan):
            if k == 2:
                for bad_f, rc in ((0, -1), (7, -1), (24, -6), (4096, -6), (-16, -1)):
                    assert lib.csdr_specbank_setup(a.h, bad_f, SLOTS, 3) == rc, bad_f
                    n_bad += 1
                assert lib.csdr_specbank_setup(a.h, F, 0, 3) == -1 and lib.csdr_specbank_setup(a.h, F, 4097, 3) == -1
                assert lib.csdr_specbank_setup(a.h, F, SLOTS, 0) == -1
            if k == 3:
                # slot 2 makes a frame per input: four inputs exceed max_frames 3; the whole call is refused, the other slots' items with it
                too_many = [(s, data[s][j]) for s, j in call] + [(2, data[2][0])]
                assert a.try_process(too_many) == -5
                assert a.try_process([(SLOTS, data[2][0])]) == -1 and a.try_process([(-1, data[2][0])]) == -1
                assert [a.frames(s) for s in range(SLOTS)] == [t.frames(s) for s in range(SLOTS)]
            if k == 4 and bank is not None:
                assert lib.csdr_specbank_process_bank(a.h, bank.h) == -4
            for s, fr in run_call(a, data, call).items():
                got[s] += fr
            for s, fr in run_call(t, data, call).items():
                twin[s] += fr
        for s in range(SLOTS):
            assert same_bytes(got[s], twin[s]), (F, s)
        assert sum(len(v) for v in got.values()) > 30 and n_bad == 5
        # the fetches' own refusals
        buf = np.empty(2 * F, np.float32)
        n = C.c_int()
        assert lib.csdr_specbank_fetch(a.h, 2, 3, buf.ctypes.data_as(C.c_void_p), buf.size, None, None) == -1
        assert lib.csdr_specbank_fetch(a.h, 2, 0, buf.ctypes.data_as(C.c_void_p), buf.size - 1, None, None) == -5
        assert lib.csdr_specbank_fetch_hold(a.h, 4, 0, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)) == -1 and n.value == 0
    finally:
        a.close(); t.close()
