"""The view bank (csdr_viewbank: viewbank_process of kernels_viewbank.hpp, include/csdr_hip.h "View bank") against
oracle.cubicsdr_chain.RefSpectrum in view mode, one model per slot, and the cases that the emulation (tests/test_viewbank_emu.py) and the device
(tests/test_gpu_viewbank.py) share.

The yardstick is the project's: rel_err < TOL = 1e-5 per frame for points, hold points and fftLastData (tests/util.py), ceiling and floor within TOL
of the ceiling, the NaN masks identical; every integer -- frames per call, hold present or not, desired_input_size, resample_bw, shift_frequency,
lastDataSize, peakReset, num_written -- exactly.  The properties (one item per call against many, independence of the slots, reset_slot, the
refusals) are bit for bit.

One slot per walk, all in one object.  Input rate 503606 (the truncated channel rate of a 2.4 MS/s stream cut into M = 4 ... rows), input
frequency FREQ.  Calls of 1, 1, 3 items and the rest; the rest is cut once more (4 + 5) so that walk (c)'s fourth setView falls between two calls."""
import functools

import numpy as np

from cubicsdr_amd.engine import ViewBank
from tests.specbank_cases import backend, check_frame, same_bytes
from tests.util import rel_err, synth_iq

TOL = 1e-5
SIZES = (16, 32, 256, 2048)           # Fi = 32: an odd bit count (lds_fft's radix-2 head); 64; 512; 4096: the limit
PEAK_SIZES = (32, 256)
RATE, RATE2, FREQ = 503606, 500000, 100000000
N_ITEMS = 14
CALLS = (1, 1, 3, 4, 5)               # items per slot and call: setView works between calls, in front of items 1, 2, 5, 9
PEAK_CALLS = (1, 1, 3, 1, 6, 14, 14)  # the setters work between calls: peak hold before items 2 and 5, a retune before item 6; 40 items
A, B, C_, D, E, F_, G1, G2, H_ = range(9)
SLOTS = 9
NOVIEW = SLOTS                        # one more slot that is never given a view


def walks(F, n_items=N_ITEMS):
    """slot -> dict(views {item: (centre, bandwidth)}, lens [samples or 0 per item] or None, rates [per item], nan item or None)"""
    Fi = 2 * F
    deep = (700 if F <= 32 else 40) * Fi
    w = {
        A: dict(views={0: (FREQ + 60000, 300000)}, lens=[3 * Fi] * n_items, nan=3),                        # (a) ratio 1 with mixing
        B: dict(views={0: (FREQ, 120000)}, lens=[Fi // 2 + 3] * n_items, nan=4),                           # (b) no mixing, two stages; primes, then slides
        C_: dict(views={0: (FREQ + 20000, 120000), 1: (FREQ + 27000, 120000), 2: (FREQ + 1000, 120000),    # (c) +7000 left, -26000 right,
                        5: (FREQ + 101000, 120000), 9: (FREQ + 101000, 120000)}, lens=[6 * Fi] * n_items), #     +100000 no move, the same centre again
        D: dict(views={0: (FREQ + 20000, 120000), 2: (FREQ + 20000, 50000), 5: (FREQ + 20000, 260000)}, lens=[6 * Fi] * n_items),   # (d) squeeze, stretch
        E: dict(views={0: (FREQ + 10000, 600)}, lens=[deep] * n_items),                                    # (e) nine stages, resampleBw 983
        F_: dict(views={0: (FREQ + 300000, 120000)}, lens=[5 * Fi] * n_items),                             # (f) out of range
        G1: dict(views={0: (FREQ + 60000, 300000)}, lens=None),                                            # (g) fed nothing
        G2: dict(views={0: (FREQ + 60000, 300000)}, lens=[0 if k in (3, 7) else 3 * Fi for k in range(n_items)]),   # (g) empty items between inputs
        H_: dict(views={0: (FREQ + 30000, 120000)}, lens=[5 * Fi] * n_items,                               # (h) rate 0 once, then another rate
                 rates=[RATE] * 6 + [0] + [RATE2] * (n_items - 7)),
    }
    for v in w.values():
        v.setdefault("rates", [RATE] * n_items)
        v.setdefault("nan", None)
    return w


def max_samples(F):
    return max(max(v["lens"]) for v in walks(F).values() if v["lens"])


@functools.lru_cache(maxsize=None)
def make_inputs(F, n_items=N_ITEMS, nan=True):
    """slot -> [complex64 arrays], cut from one seeded carriers-over-noise stream per slot (shared by every check: not to be written to)"""
    data = {}
    for s, v in walks(F, n_items).items():
        if v["lens"] is None:
            data[s] = None
            continue
        x = synth_iq(sum(v["lens"]), float(RATE), FREQ, [("NBFM", FREQ + 55000.0 + 900.0 * s), ("AM", FREQ + 10150.0), ("NBFM", FREQ - 31000.0)], seed=700 + 13 * s + F)
        cut, at = [], 0
        for n in v["lens"]:
            cut.append(x[at:at + n].copy())
            at += n
        if nan and v["nan"] is not None:
            c = cut[v["nan"]]
            c[len(c) // 8] = np.complex64(complex(np.nan, 0.25))          # (inside the prefix the input consumes, and out of reach of the next input's first window)
        for c in cut:
            c.setflags(write=False)
        data[s] = cut
    return data


def _model(F, hide_dc=False):
    from oracle.cubicsdr_chain import RefSpectrum

    class Ref(RefSpectrum):
        num_written = 0

        def _view_input(self, x, frequency, sample_rate):
            out = super()._view_input(x, frequency, sample_rate)
            if out is not None:
                self.num_written = len(out)
            return out
    m = Ref(backend(), F)
    if hide_dc:
        m.set_hide_dc(True, 0, 0, 0)            # (before setView: the setter of the model also takes the three frequencies)
    return m


def model_info(m):
    return dict(desired_input_size=m.desired_input_size, resample_bw=getattr(m, "resample_bw", 0), shift_frequency=m.shift_frequency,
                last_data_size=getattr(m, "last_size", 0), peak_reset=m.peak_reset, num_written=m.num_written)


def run_model(F, w, data, n_items, peak_events=None, hide_dc=False, extra_views=None):
    """-> {slot: [per item: None (no input), or dict(frame or None, info, last)]}; peak_events {item: on}; extra_views {item: {slot: view}}"""
    ms = {s: _model(F, hide_dc) for s in w}
    out = {s: [] for s in w}
    for k in range(n_items):
        if peak_events and k in peak_events:
            for m in ms.values():
                m.set_peak_hold(peak_events[k])
        for s, v in w.items():
            view = v["views"].get(k)
            if extra_views and s in extra_views.get(k, {}):
                view = extra_views[k][s]
            if view:
                ms[s].set_view(True, *view)
            if data[s] is None or len(data[s][k]) == 0:
                out[s].append(None)
                continue
            fr = ms[s].process_input(data[s][k], FREQ, v["rates"][k])
            last = ms[s].last.copy() if hasattr(ms[s], "last") else np.zeros(2 * F, np.complex64)
            out[s].append(dict(frame=fr, info=model_info(ms[s]), last=last))
    return out


@functools.lru_cache(maxsize=None)
def model_main(F):
    return run_model(F, walks(F), make_inputs(F), N_ITEMS)


def new_bank(ctx, F, max_frames=max(CALLS), ms=None):
    return ViewBank(ctx, F, SLOTS + 1, max_frames, ms or max_samples(F))


def call_plan(w, data, calls, order="slot", only=None):
    """[(first item, [(slot, item)])] per call"""
    plan, at = [], 0
    slots = [s for s in sorted(w) if data[s] is not None and (only is None or s in only)]
    for per in calls:
        if order == "slot":
            plan.append((at, [(s, k) for s in slots for k in range(at, at + per)]))
        else:
            plan.append((at, [(s, k) for k in range(at, at + per) for s in reversed(slots)]))
        at += per
    return plan


def apply_views(vb, w, k0, k1, extra_views=None):
    """the setView calls that fall in front of items k0 .. k1 - 1 (by construction only in front of k0)"""
    for s, v in w.items():
        for k in range(k0, k1):
            view = v["views"].get(k)
            if extra_views and s in extra_views.get(k, {}):
                view = extra_views[k][s]
            if view:
                assert k == k0, (s, k, k0)
                vb.set_view(s, *view)


def run_call(vb, w, data, call):
    """one process call -> {slot: [(points, ceiling, floor, hold or None)]}"""
    vb.process([(s, data[s][k], FREQ, w[s]["rates"][k]) for s, k in call])
    out = {}
    for s in range(vb.max_slots):
        out[s] = []
        for j in range(vb.frames(s)):
            p, ce, fl = vb.fetch(s, j)
            out[s].append((p, ce, fl, vb.fetch_hold(s, j)))
    return out


def run_plan(vb, w, data, plan, before_call=None, extra_views=None):
    """-> ({slot: [frames in order]}, {slot: [frames per call]}) over all calls of the plan; before_call(k, first item) runs in front of call k"""
    got = {s: [] for s in range(vb.max_slots)}
    per = {s: [] for s in range(vb.max_slots)}
    for k, (k0, call) in enumerate(plan):
        if before_call:
            before_call(k, k0)
        k1 = max(i for _, i in call) + 1
        apply_views(vb, w, k0, k1, extra_views)
        for s, fr in run_call(vb, w, data, call).items():
            got[s] += fr
            per[s].append(len(fr))
    return got, per


def check_state(vb, s, want_item, where):
    """the slot's integers and fftLastData behind a call against the model behind the slot's last item of that call"""
    assert vb.slot_info(s) == want_item["info"], (where, vb.slot_info(s), want_item["info"])
    last, wl = vb.fetch_last(s), want_item["last"]
    bad = np.isnan(wl.view(np.float32))
    assert np.array_equal(np.isnan(last.view(np.float32)), bad), (where, "fftLastData NaN")
    if not bad.all():
        e = rel_err(last.view(np.float32)[~bad], wl.view(np.float32)[~bad])
        assert e < TOL, (where, "fftLastData", e)
        return e
    return 0.0


def check_walk(vb, w, data, want, plan, before_call=None, extra_views=None):
    """a plan call by call against the model: frames per call, every frame, and behind every call the integers and fftLastData.
    -> (frames checked, worst error)"""
    n, worst = 0, 0.0
    cursor = {s: 0 for s in w}
    for k, (k0, call) in enumerate(plan):
        if before_call:
            before_call(k, k0)
        k1 = max(i for _, i in call) + 1
        apply_views(vb, w, k0, k1, extra_views)
        got = run_call(vb, w, data, call)
        for s in w:
            items = [want[s][i] for i in range(k0, k1)]
            frames = [it["frame"] for it in items if it is not None and it["frame"] is not None]
            assert len(got[s]) == len(frames), (s, k, len(got[s]), len(frames))
            for j, (g, f) in enumerate(zip(got[s], frames)):
                worst = max(worst, check_frame(g, f, (vb.fft_size, s, k, j)))
                n += 1
            fed = [it for it in items if it is not None]
            if fed:
                worst = max(worst, check_state(vb, s, fed[-1], (vb.fft_size, s, k)))
            cursor[s] = k1
    return n, worst


def frame_counts(want):
    return {s: sum(1 for it in v if it is not None and it["frame"] is not None) for s, v in want.items()}


# what the model gives, pinned: a frame for every input of (a), (c), (f) and of (g)'s fed slot; 13 of 14 for (b), whose first input primes; (e) makes a
# frame per input with inputs longer than desiredInputSize (F <= 32) and from the second input on with short ones (the first primes to Fi at once);
# (d) loses one input to the late priming (the first whose num_written falls short of Fi, behind the zoom to 50000); (h) loses the input with rate 0
def expected_counts(F):
    return {A: 14, B: 13, C_: 14, D: 13, E: 14 if F <= 32 else 13, F_: 14, G1: 0, G2: 12, H_: 13}


def check_against_model(ctx, F):
    w, data, want = walks(F), make_inputs(F), model_main(F)
    counts = frame_counts(want)
    for s, c in expected_counts(F).items():
        assert counts[s] == c, (F, s, counts)
    # the NaN inputs: (a) replaces its window with every input -- finite again two frames later (:494-497); (b) keeps the sample while it slides
    fa = [it["frame"] for it in want[A]]
    masks = [np.isnan(f[0][1::2]) for f in fa]
    k = w[A]["nan"]
    assert not masks[k].any() and masks[k + 1].all() and not any(m.any() for m in masks[k + 2:]), [int(m.sum()) for m in masks]
    assert any(np.isnan(it["frame"][0]).any() for it in want[B] if it["frame"] is not None)
    # the walks take the branches they are named for
    infos = {s: [it["info"] for it in want[s] if it is not None] for s in w}
    assert {i["resample_bw"] for i in infos[B]} == {125901} and {i["resample_bw"] for i in infos[E]} == {983}
    assert [i["shift_frequency"] for i in infos[C_]][:3] == [20000, 27000, 1000] and infos[C_][-1]["shift_frequency"] == 101000
    assert {i["shift_frequency"] for i in infos[F_]} == {0} and all(i["peak_reset"] == 30 for i in infos[F_])
    assert [i["resample_bw"] for i in infos[D]][1:6:2] == [125901, 62950, 503606]
    assert infos[H_][5]["resample_bw"] == 125901 and infos[H_][7]["resample_bw"] == 125000 and infos[H_][6] == infos[H_][5] | {"peak_reset": infos[H_][6]["peak_reset"]}
    vb = new_bank(ctx, F)
    try:
        n, worst = check_walk(vb, w, data, want, call_plan(w, data, CALLS))
        assert vb.frames(G1) == 0 and vb.slot_info(G1)["last_data_size"] == 0
    finally:
        vb.close()
    print("view bank F = %d: %d frames against the model, worst rel_err %.3g, frames per walk %s" % (F, n, worst, counts))
    return n, worst


def peak_walks(F, n_items):
    Fi = 2 * F
    return {
        0: dict(views={0: (FREQ + 60000, 300000), 6: (FREQ + 70000, 300000)}, lens=[3 * Fi] * n_items, rates=[RATE] * n_items, nan=None),
        1: dict(views={0: (FREQ, 120000)}, lens=[Fi // 2 + 3] * n_items, rates=[RATE] * n_items, nan=None),
        2: dict(views={0: (FREQ + 20000, 120000), 6: (FREQ + 27000, 120000)}, lens=[6 * Fi] * n_items, rates=[RATE] * n_items, nan=None),
    }


def check_peak_hold(ctx, F):
    """peak hold enabled before item 2 and again before item 5, a retune before item 6 re-arms the countdown, which runs out inside the 40 items"""
    n_items = sum(PEAK_CALLS)
    w = peak_walks(F, n_items)
    data = {}
    for s, v in w.items():
        x = synth_iq(sum(v["lens"]), float(RATE), FREQ, [("NBFM", FREQ + 55000.0), ("AM", FREQ + 10150.0)], seed=31 + s + F)
        data[s] = [x[k * v["lens"][0]:(k + 1) * v["lens"][0]] for k in range(n_items)]
    events = {2: True, 5: True}
    want = run_model(F, w, data, n_items, events)
    vb = ViewBank(ctx, F, 3, max(PEAK_CALLS), 6 * 2 * F)
    try:
        assert not vb.get_peak_hold()
        n, worst = check_walk(vb, w, data, want, call_plan(w, data, PEAK_CALLS), lambda k, k0: vb.set_peak_hold(True) if k0 in events else None)
        assert vb.get_peak_hold()
    finally:
        vb.close()
    held = {s: [k for k, it in enumerate(want[s]) if it["frame"] is not None and it["frame"][3] is not None] for s in w}
    # slots 0 and 2 make a frame per input: hold behind the first reset (items 3, 4), none while the countdown of the second enable and of the
    # retune runs (the retune sets 30 behind item 6's own decrement: it ends in front of item 36), hold again from item 37 on; slot 1 is never
    # retuned: its countdown started at item 5
    assert held[0] == [3, 4] + list(range(37, n_items)) and held[2] == held[0], held
    assert held[1] == [3, 4] + list(range(35, n_items)), held[1]
    return sum(len(v) for v in held.values())


def check_hide_dc(ctx, F):
    """hideDC on: the input frequency inside the view in (a), outside it in (f); the kernel overwrites the span in points and hold points"""
    n_items = 6
    w = {s: v for s, v in walks(F, n_items).items() if s in (A, F_)}
    data = {s: make_inputs(F, N_ITEMS, False)[s][:n_items] for s in w}
    events = {1: True}
    want = run_model(F, w, data, n_items, events, hide_dc=True)
    plain = run_model(F, w, data, n_items, events, hide_dc=False)
    vb = new_bank(ctx, F, 3)
    try:
        vb.set_hide_dc(True)
        n, worst = check_walk(vb, w, data, want, call_plan(w, data, (1, 1, 1, 3)), lambda k, k0: vb.set_peak_hold(True) if k0 in events else None)
    finally:
        vb.close()
    changed = [not np.array_equal(a["frame"][0], b["frame"][0]) for a, b in zip(want[A], plain[A])]
    assert all(changed[1:]), changed                                 # inside the view: (a)'s frames differ from the unhidden ones (the first is flat: second averager still 0)
    assert all(np.array_equal(a["frame"][0], b["frame"][0]) for a, b in zip(want[F_], plain[F_]))      # outside: nothing to hide
    assert any(it["frame"][3] is not None for it in want[A])         # hold points went through it too
    return n


def _final_state(vb, slots):
    return {s: (vb.slot_info(s), vb.fetch_last(s).tobytes()) for s in slots}


def check_properties(ctx, F):
    """bit for bit: one item per call against many per call; a slot alone against the slot among the others in two interleavings; reset_slot"""
    w, data = walks(F), make_inputs(F)
    fed = [s for s in sorted(w) if data[s] is not None]
    a = new_bank(ctx, F)
    many, many_per = run_plan(a, w, data, call_plan(w, data, CALLS))
    many_state = _final_state(a, fed)
    a.close()
    b = new_bank(ctx, F, 1)
    single, _ = run_plan(b, w, data, call_plan(w, data, (1,) * N_ITEMS))
    single_state = _final_state(b, fed)
    b.close()
    c = new_bank(ctx, F)
    inter, _ = run_plan(c, w, data, call_plan(w, data, CALLS, order="item"))
    inter_state = _final_state(c, fed)
    c.close()
    for s in range(SLOTS):
        assert same_bytes(many[s], single[s]), (F, s, "one item per call")
        assert same_bytes(many[s], inter[s]), (F, s, "interleaving")
    assert many_state == single_state == inter_state
    # the frames of (b), (d), (h): which items give one is the model's pattern exactly (one item per call: a frame or none per call)
    want = model_main(F)
    for s in (A, C_, G2):
        alone_w = {k: v for k, v in w.items()}
        d = new_bank(ctx, F)
        got, _ = run_plan(d, alone_w, data, call_plan(w, data, CALLS, only=(s,)))
        st = _final_state(d, (s,))
        d.close()
        assert same_bytes(many[s], got[s]), (F, s, "alone")
        assert st[s] == many_state[s], (F, s, "alone: state")
        assert all(not got[k] for k in range(SLOTS) if k != s)
    b = new_bank(ctx, F, 1)
    _, per1 = run_plan(b, w, data, call_plan(w, data, (1,) * N_ITEMS, only=(B, D, H_)))
    b.close()
    for s in (B, D, H_):
        assert per1[s] == [int(it is not None and it["frame"] is not None) for it in want[s]], (F, s, per1[s])
    # reset_slot: slot (a), whose view never changes, starts over with its own inputs 0 .. 8 while the others go on with 5 .. 13
    e = new_bank(ctx, F)
    first, first_per = run_plan(e, w, data, call_plan(w, data, CALLS[:3]))
    e.reset_slot(A)
    second = {s: [] for s in range(e.max_slots)}
    for k0, per in ((5, 4), (9, 5)):
        apply_views(e, {s: v for s, v in w.items() if s != A}, k0, k0 + per)
        call = [(s, k) for s in fed if s != A for k in range(k0, k0 + per)]
        vals = [(s, data[s][k], FREQ, w[s]["rates"][k]) for s, k in call] + [(A, data[A][k - 5], FREQ, RATE) for k in range(k0, k0 + per)]
        e.process(vals)
        for s in range(e.max_slots):
            second[s] += [(e.fetch(s, j) + (e.fetch_hold(s, j),)) for j in range(e.frames(s))]
    e.close()
    n9 = sum(many_per[A][:4])                                         # frames of (a)'s items 0 .. 8
    assert same_bytes(second[A], many[A][:n9]), (F, "reset_slot")
    assert same_bytes(first[A], many[A][:len(first[A])])
    for s in fed:
        if s != A:
            assert same_bytes(first[s] + second[s], many[s]), (F, s, "neighbour of a reset slot")


def check_refusals(ctx, F, post=None):
    """every refusal against an undisturbed twin: bad sizes, an eleven-stage view, max_samples or max_frames exceeded, a slot without a view, a
    negative rate, process_post before an execute (`post`: a channelizer that has not executed).  Each is refused with its code and changes
    nothing: the valid calls around them equal the same calls on the twin, and so do the slots' integers and fftLastData at the end"""
    import cubicsdr_amd.hip as H
    w, data = walks(F), make_inputs(F)
    fed = [s for s in sorted(w) if data[s] is not None]
    lib = H.lib()
    ms = max_samples(F)
    a, t = new_bank(ctx, F), new_bank(ctx, F)
    try:
        plan = call_plan(w, data, CALLS)
        got, twin = {s: [] for s in range(a.max_slots)}, {s: [] for s in range(a.max_slots)}
        n_bad = 0
        for k, (k0, call) in enumerate(plan):
            k1 = max(i for _, i in call) + 1
            apply_views(a, w, k0, k1)
            apply_views(t, w, k0, k1)
            valid = [(s, data[s][i], FREQ, w[s]["rates"][i]) for s, i in call]
            if k == 2:
                for bad_f, rc in ((0, -1), (7, -1), (24, -6), (4096, -6), (-16, -1)):
                    assert lib.csdr_viewbank_setup(a.h, bad_f, SLOTS + 1, 5, ms) == rc, bad_f
                    n_bad += 1
                for args in ((F, 0, 5, ms), (F, 4097, 5, ms), (F, SLOTS + 1, 0, ms), (F, SLOTS + 1, 5, 0)):
                    assert lib.csdr_viewbank_setup(a.h, *args) == -1, args
                    n_bad += 1
                assert a.try_set_view(A, FREQ, 0) == -1 and a.try_set_view(A, FREQ, -5) == -1 and a.try_set_view(SLOTS + 1, FREQ, 1000) == -1
            if k == 3:
                # bandwidth 200 on 503606: resampleBw 245, eleven half-band stages; the whole call is refused, the other slots' items with it
                a.set_view(G1, FREQ + 60000, 200)
                assert a.try_process(valid + [(G1, data[A][0], FREQ, RATE)]) == -6
                a.set_view(G1, *w[G1]["views"][0])
                assert a.try_process(valid + [(A, np.zeros(ms + 1, np.complex64), FREQ, RATE)]) == -5          # max_samples
                assert a.try_process(valid + [(A, data[A][0], FREQ, RATE)] * 6) == -5                           # max_frames: (a) makes a frame per input
                assert a.try_process(valid + [(NOVIEW, data[A][0], FREQ, RATE)]) == -4                          # never given a view
                assert a.try_process(valid + [(A, data[A][0], FREQ, -1)]) == -1
                assert a.try_process([(SLOTS + 1, data[A][0], FREQ, RATE)]) == -1 and a.try_process([(-1, data[A][0], FREQ, RATE)]) == -1
                n_bad += 7
                assert [a.frames(s) for s in range(a.max_slots)] == [t.frames(s) for s in range(a.max_slots)]
            if k == 4 and post is not None:
                assert a.try_process_post(post, [A], [0]) == -4
                n_bad += 1
            for s, fr in run_call(a, w, data, call).items():
                got[s] += fr
            for s, fr in run_call(t, w, data, call).items():
                twin[s] += fr
        for s in range(a.max_slots):
            assert same_bytes(got[s], twin[s]), (F, s)
        assert _final_state(a, fed) == _final_state(t, fed)
        assert sum(len(v) for v in got.values()) > 80 and n_bad == 16 + (post is not None)
        # the fetches' own refusals
        import ctypes as C
        buf = np.empty(4 * F, np.float32)
        n = C.c_int()
        assert lib.csdr_viewbank_fetch(a.h, A, 5, buf.ctypes.data_as(C.c_void_p), buf.size, None, None) == -1
        assert lib.csdr_viewbank_fetch(a.h, A, 0, buf.ctypes.data_as(C.c_void_p), 2 * F - 1, None, None) == -5
        assert lib.csdr_viewbank_fetch_hold(a.h, G1, 0, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)) == -1 and n.value == 0
        assert lib.csdr_viewbank_fetch_last(a.h, A, buf.ctypes.data_as(C.c_void_p), 4 * F - 1) == -5
    finally:
        a.close(); t.close()
