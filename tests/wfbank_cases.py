"""The waterfall bank (csdr_wfbank: kernels_wfbank.hpp, csdr_wfbank.hip, include/csdr_hip.h "Waterfall bank") against the two yardsticks the
waterfall already has -- one PanelModel per slot with np_view for the tiles (tests/waterfall_cases.py, tests/waterfall_view_cases.py), and one
csdr_waterfall per slot fed the same lines -- and the cases that the emulation (tests/test_wfbank_emu.py) and the device
(tests/test_gpu_wfbank.py) share.  Every comparison is byte for byte; no tolerance appears anywhere.

Six slots, lines = 7, max_pending = 32:
  (a) 3, 5, 7, 1, 20 lines between updates: the worked example of csdr_hip.h (H G F C B E D, offset 5), then the wrap crossed with more pending lines
      than the ring has rows; one of its lines is made of the quantiser's special values
  (b) one line per call; its first line after the textures exist is NULL and repeats the points of its dropped step
  (c) the pair layout (2 fft_size floats) throughout
  (d) never stepped: offset -1, no textures, a zero tile
  (e) two dropped steps without points, then a NULL line as its very first (a row of index 0), a wrong-length line directly behind a good one in
      the same call, and NULL lines behind those
  (f) starts three updates late, so its offset differs from its neighbours' from then on"""
import ctypes as C

import numpy as np

import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import Waterfall, WaterfallBank
from tests import waterfall_cases as WK
from tests.waterfall_cases import PanelModel, np_table, special_values, stops256
from tests.waterfall_view_cases import np_columns, np_rows, np_view

F32 = np.float32
LINEAR, PEAK = 0, 1
MODES = (("linear", LINEAR), ("peak", PEAK))
FFT_SIZES = (2, 16, 30, 601, 2048)
VIEW_SIZES = (16, 30, 601, 2048)
LINES, SLOTS, MAX_PENDING = 7, 6, 32
A, B, Cc, D, E, Fs = range(6)
LIFE_COUNTS = WK.LIFE_COUNTS                # 3, 5, 7, 1, 20


# ------------------------------------------------------------------------------------------------------------------ the calls
def plan(fft_size):
    """-> [turn], a turn = [(slot, lines or None, n_lines)] in the order of one step call; an update follows every turn.  `lines` is a float32 array
    [n_lines, floats per line]."""
    rng = {s: np.random.default_rng(7000 + 31 * s + fft_size) for s in range(SLOTS)}

    def plain(s, n):
        return rng[s].uniform(-0.2, 1.2, (n, fft_size)).astype(F32)

    def pairs(s, n):
        y = plain(s, n)
        return np.stack([rng[s].uniform(0, 1, y.shape).astype(F32), y], axis=2).reshape(n, 2 * fft_size)

    def const(values):
        return np.stack([np.full(fft_size, v, F32) for v in values])
    val = [F32((i + 1) * 10 / 255.0 + 0.001) for i in range(8)]          # A .. H of the worked example: eight different bytes, none of them 0
    wrong = 5 if fft_size not in (5, 10) else 6
    turns = []
    # turn 0: every step is dropped (no textures yet); (a) a good line and a wrong-length one behind it, (e) two steps without points
    turns.append([(A, plain(A, 1), 1), (E, None, 1), (B, plain(B, 1), 1), (A, np.full((1, wrong), 0.5, F32), 1), (Cc, pairs(Cc, 2), 2), (E, None, 1)])
    for k, n in enumerate(LIFE_COUNTS):
        t = []
        a = const(val[:3]) if k == 0 else const(val[3:]) if k == 1 else plain(A, n)
        if k == 2:
            a[3] = np.resize(special_values()[::-1], fft_size)            # (reversed: NaN, the infinities, -0 and the 0.99 edges come first)
        t.append((A, a, n))
        t.append((B, None, 1) if k == 0 else (B, plain(B, 1), 1))
        t.append((Cc, pairs(Cc, k % 3 + 1), k % 3 + 1))
        if k == 0:
            t += [(E, None, 1), (E, plain(E, 2), 2), (E, np.full((1, wrong), 0.25, F32), 1), (E, None, 2)]
        elif k == 3:
            t += [(E, None, 1), (E, pairs(E, 1), 1), (E, np.zeros((2, 3 * fft_size), F32), 2)]
        else:
            t.append((E, plain(E, 2), 2))
        if k >= 2:                                                        # (f): the updates behind turns 0, 1 and 2 have passed
            t.append((Fs, plain(Fs, (2, 4, 9)[k - 2]), (2, 4, 9)[k - 2]))
        turns.append(t)
    return turns


def interleave(turn, how):
    """the items of a turn in another order that keeps every slot's own: 0 as planned, 1 slot by slot, 2 reversed slot order"""
    if how == 0:
        return list(turn)
    order = sorted({it[0] for it in turn}, reverse=(how == 2))
    return [it for s in order for it in turn if it[0] == s]


def model_step(models, items):
    """the items through the models -> lines taken per item"""
    taken = []
    for slot, lines, n in items:
        m, t = models[slot], 0
        for l in range(n):
            if lines is not None:
                m.set_points(lines[l])
            t += m.step()
        taken.append(t)
    return taken


def same_state(wb, models, where=""):
    for s, m in enumerate(models):
        assert wb.lines_buffered(s) == m.lines_buffered, (where, s)
        if m.tex_init:
            assert wb.offset(s, 0) == m.ofs[0] and wb.offset(s, 1) == m.ofs[1], (where, s, wb.offset(s, 0), m.ofs)
            for j in range(2):
                got = wb.fetch_index(s, j)
                assert np.array_equal(got, m.tex[j]), (where, s, j, np.argwhere(got != m.tex[j])[:8])
        else:
            assert wb.offset(s, 0) == -1 and wb.offset(s, 1) == -1, (where, s)
            buf = np.empty(LINES * max(wb.half, 1), np.uint8)
            assert H.lib().csdr_wfbank_fetch_index(wb.h, s, 0, buf.ctypes.data_as(C.c_void_p), buf.size) == -4


def same_banks(x, y, where=""):
    """two banks hold the same bytes: lines_buffered, offsets and textures of every slot, and -- where there is something to filter -- the atlas"""
    for s in range(SLOTS):
        assert x.lines_buffered(s) == y.lines_buffered(s), (where, s)
        for j in range(2):
            assert x.offset(s, j) == y.offset(s, j), (where, s, j)
            if x.offset(s, j) >= 0:
                assert np.array_equal(x.fetch_index(s, j), y.fetch_index(s, j)), (where, s, j)
    if x.fft_size >= 4:
        assert np.array_equal(x.view(SLOTS, 5, 3, "linear", 2), y.view(SLOTS, 5, 3, "linear", 2)), where


def new_bank(ctx, fft_size):
    return WaterfallBank(ctx, fft_size, LINES, SLOTS, MAX_PENDING), [PanelModel(fft_size, LINES) for _ in range(SLOTS)]


# ------------------------------------------------------------------------------------------------------------------ the cases
def check_life_cycle(ctx, fft_size):
    """the plan, one step call per turn: lines taken per item, then lines_buffered, both offsets and both textures of every slot after every update"""
    wb, models = new_bank(ctx, fft_size)
    half = fft_size // 2
    n = 0
    try:
        wb.update()                                       # before any step: nothing happens anywhere
        same_state(wb, models, "fresh")
        for k, turn in enumerate(plan(fft_size)):
            assert wb.step(turn) == model_step(models, turn), k
            for s, m in enumerate(models):
                assert wb.lines_buffered(s) == m.lines_buffered, (k, s)
            wb.update()
            for m in models:
                m.update()
            same_state(wb, models, k)
            n += 1
            if k == 1:                                    # A, B, C -> rows 3, 4, 5 = C, B, A, offset 3
                assert wb.offset(A, 0) == 3 and [int(r[0]) for r in wb.fetch_index(A, 0)][3:6] == [int(WK.np_quantise(v)) for v in turn[0][1][::-1, 0]]
            if k == 2:                                    # D .. H -> rows 0 .. 6 = H, G, F, C, B, E, D, offset 5
                val = [F32((i + 1) * 10 / 255.0 + 0.001) for i in range(8)]
                byte = dict(zip("ABCDEFGH", (int(WK.np_quantise(np.array([v]))[0]) for v in val)))
                assert len(set(byte.values())) == 8 and 0 not in byte.values()
                assert wb.offset(A, 0) == 5 and wb.offset(A, 1) == 5
                for j in range(2):
                    t = wb.fetch_index(A, j)
                    assert [int(r[0]) for r in t] == [byte[c] for c in "HGFCBED"] and (t == t[:, :1]).all()
            if k == 1:
                e0 = wb.fetch_index(E, 0)
                assert not e0[LINES - 2].any() and (e0[LINES - 3].any() or half < 8)      # the NULL line, then the first good line
                assert wb.fetch_index(B, 0)[LINES - 2].any() or half < 8                  # (b)'s NULL line repeated its dropped step's points
                assert np.array_equal(e0[LINES - 4], e0[LINES - 5]) and np.array_equal(e0[LINES - 5], e0[LINES - 6])      # good line 2, the wrong-length line, NULL
        # (d) was never stepped; (f) started late and sits elsewhere in its ring than (a); every ring has wrapped or not by its own history
        assert wb.offset(D, 0) == -1 and models[Fs].ofs[0] != models[A].ofs[0]
        assert len({m.ofs[0] for m in models if m.tex_init}) >= 3
    finally:
        wb.close()
    return n


def check_one_item_per_call(ctx, fft_size):
    """one item per call against all items in one call, and the item list in two more interleavings: the same bytes everywhere"""
    banks = [WaterfallBank(ctx, fft_size, LINES, SLOTS, MAX_PENDING) for _ in range(4)]
    try:
        for k, turn in enumerate(plan(fft_size)):
            want = banks[0].step(turn)
            got = [banks[1].step([it])[0] for it in turn]
            assert got == want, k
            for how in (1, 2):
                ordered = interleave(turn, how)
                assert sorted(zip([it[0] for it in ordered], banks[1 + how].step(ordered))) == sorted(zip([it[0] for it in turn], want)), (k, how)
            for b in banks:
                b.update()
            for b in banks[1:]:
                same_banks(banks[0], b, k)
    finally:
        for b in banks:
            b.close()


def check_slot_alone(ctx, fft_size, slots=(A, E, Fs)):
    """a slot alone in a bank against the slot among the others: what its neighbours are fed, and whether they are fed at all, changes no byte of it"""
    full = WaterfallBank(ctx, fft_size, LINES, SLOTS, MAX_PENDING)
    alone = {s: WaterfallBank(ctx, fft_size, LINES, SLOTS, MAX_PENDING) for s in slots}
    try:
        for k, turn in enumerate(plan(fft_size)):
            full.step(turn)
            full.update()
            for s, b in alone.items():
                b.step([it for it in turn if it[0] == s])
                b.update()
                assert b.lines_buffered(s) == full.lines_buffered(s) and b.offset(s, 0) == full.offset(s, 0) and b.offset(s, 1) == full.offset(s, 1), (k, s)
                for j in range(2):
                    if b.offset(s, j) >= 0:
                        assert np.array_equal(b.fetch_index(s, j), full.fetch_index(s, j)), (k, s, j)
                for o in range(SLOTS):
                    assert o == s or b.offset(o, 0) == -1
    finally:
        full.close()
        for b in alone.values():
            b.close()


def check_reset_slot(ctx, fft_size, slot=B, at=3):
    """reset_slot before turn `at`: the slot goes on as a fresh panel (the model, and a fresh object fed the rest of its items) while its neighbours
    go on as if nothing had happened"""
    wb, models = new_bank(ctx, fft_size)
    fresh = WaterfallBank(ctx, fft_size, LINES, SLOTS, MAX_PENDING)
    try:
        for k, turn in enumerate(plan(fft_size)):
            if k == at:
                # with lines waiting: they go too
                extra = [(slot, np.full((2, fft_size), 0.5, F32), 2)]
                assert wb.step(extra) == model_step(models, extra) == [2]
                wb.reset_slot(slot)
                models[slot] = PanelModel(fft_size, LINES)
                same_state(wb, models, "reset")
            if k >= at:
                # NULL lines first, one dropped and one stored: the points are zero again, the stored row is a row of index 0
                turn = [((s, None, n) if (s == slot and k <= at + 1) else (s, l, n)) for s, l, n in turn]
                fresh.step([it for it in turn if it[0] == slot])
                fresh.update()
            assert wb.step(turn) == model_step(models, turn), k
            wb.update()
            for m in models:
                m.update()
            same_state(wb, models, k)
            if k >= at:
                assert fresh.offset(slot, 0) == wb.offset(slot, 0)
                for j in range(2):
                    if wb.offset(slot, j) >= 0:
                        assert np.array_equal(fresh.fetch_index(slot, j), wb.fetch_index(slot, j)), (k, j)
        assert wb.offset(slot, 0) >= 0 and wb.offset(slot, 0) != wb.offset(A, 0) and not wb.fetch_index(slot, 0)[LINES - 2].any()
    finally:
        wb.close(); fresh.close()


def check_setup_keeps_points(ctx, sizes=((16, 30), (601, 16), (30, 30))):
    """setup per slot is :13-24: lines_buffered cleared, textures gone, the points kept -- resized, new ones zero -- also when the slot count changes;
    a slot the object did not have before starts with zero points"""
    for f0, f1 in sizes:
        wb, models = new_bank(ctx, f0)
        try:
            rng = np.random.default_rng(f0 + f1)
            first = [(s, rng.uniform(0.1, 0.9, (1, f0)).astype(F32), 1) for s in (0, 2, 3)]
            for _ in range(2):                            # dropped, then stored: slot 3 holds pending lines and textures when the setup comes
                assert wb.step(first) == model_step(models, first)
                wb.update()
                for m in models:
                    m.update()
            wb.step([(3, None, 1)]); model_step(models, [(3, None, 1)])
            wb.setup(f1, LINES + 1, SLOTS + 2, MAX_PENDING)
            for m in models:
                m.setup(f1, LINES + 1)
            models += [PanelModel(f1, LINES + 1) for _ in range(2)]
            assert [wb.lines_buffered(s) for s in range(SLOTS + 2)] == [0] * (SLOTS + 2) and [wb.offset(s, 0) for s in range(SLOTS + 2)] == [-1] * (SLOTS + 2)
            again = [(s, None, 1) for s in (0, 1, 2, 3, SLOTS + 1)]
            for _ in range(2):
                assert wb.step(again) == model_step(models, again)
                wb.update()
                for m in models:
                    m.update()
            for s in (0, 1, 2, 3, SLOTS + 1):
                assert wb.offset(s, 0) == models[s].ofs[0] == LINES - 1
                for j in range(2):
                    got = wb.fetch_index(s, j)
                    assert np.array_equal(got, models[s].tex[j]), (f0, f1, s, j)
            assert wb.fetch_index(0, 0)[LINES - 1].any() and not wb.fetch_index(1, 0).any() and not wb.fetch_index(SLOTS + 1, 1).any()
        finally:
            wb.close()


def _rc_step(wb, items):
    rc, taken = wb.try_step(items)
    return rc, taken


def check_refusals(ctx, fft_size):
    """every refusal against an undisturbed twin: nothing is taken, nothing changes, in no slot -- and the calls after it give the twin's bytes"""
    wb = WaterfallBank(ctx, fft_size, LINES, SLOTS, MAX_PENDING)
    twin = WaterfallBank(ctx, fft_size, LINES, SLOTS, MAX_PENDING)
    lib = H.lib()
    rng = np.random.default_rng(88 + fft_size)
    turns = plan(fft_size)
    try:
        for b in (wb, twin):
            for turn in turns[:3]:
                b.step(turn)
                b.update()
            b.step([(A, np.full((30, fft_size), 0.3, F32), 30), (B, np.full((1, fft_size), 0.7, F32), 1)])
        line = rng.uniform(0, 1, (3, fft_size)).astype(F32)
        # 30 lines wait in (a), 3 more would exceed max_pending = 32: nothing is taken in ANY slot
        rc, taken = _rc_step(wb, [(B, line[:1], 1), (A, line, 3), (Cc, line[:2], 2), (Fs, line[:1], 1)])
        assert rc == -5 and taken == [0, 0, 0, 0]
        rc, taken = _rc_step(wb, [(A, None, 3)])                              # (a repeat is refused alike)
        assert rc == -5 and taken == [0]
        rc, taken = _rc_step(wb, [(A, line[:2], 2), (A, line[:1], 1)])        # (the items of a slot add up)
        assert rc == -5 and taken == [0, 0]
        # a slot out of range
        for bad in (SLOTS, -1):
            rc, taken = _rc_step(wb, [(B, line[:1], 1), (bad, line[:1], 1)])
            assert rc == -1 and taken == [0, 0], bad
        # the bad setup sizes
        for args in ((1, LINES, SLOTS, 4), (4097, LINES, SLOTS, 4), (fft_size, 1, SLOTS, 4), (fft_size, 4097, SLOTS, 4), (fft_size, LINES, 0, 4),
                     (fft_size, LINES, 4097, 4), (fft_size, LINES, SLOTS, 0)):
            assert lib.csdr_wfbank_setup(wb.h, *args) == -1, args
        assert lib.csdr_wfbank_reset_slot(wb.h, SLOTS) == -1
        same_banks(wb, twin, "after the refused steps")
        if fft_size >= 4:
            pic = wb.view([2, 0, 1], 6, 4, "peak", 2, fetch=True)
            wb.view([2, 0, 1], 6, 4, "peak", 2, fetch=False)
            ptr = wb.device_view()
            assert ptr[1:] == (12, 8)
            n = 3
            lst = (C.c_int * n)(2, 0, 1)
            for cols in (0, n + 1):
                assert lib.csdr_wfbank_render(wb.h, lst, n, 6, 4, PEAK, cols, None, 0) == -1, cols
            assert lib.csdr_wfbank_render(wb.h, lst, n, 1, 4, PEAK, 1, None, 0) == -1
            assert lib.csdr_wfbank_render(wb.h, lst, n, 6, 0, LINEAR, 1, None, 0) == -1
            assert lib.csdr_wfbank_render(wb.h, lst, n, 6, 4, 2, 1, None, 0) == -1
            assert lib.csdr_wfbank_render(wb.h, lst, 0, 6, 4, PEAK, 1, None, 0) == -1
            assert lib.csdr_wfbank_render(wb.h, (C.c_int * n)(2, SLOTS, 1), n, 6, 4, PEAK, 1, None, 0) == -1
            assert lib.csdr_wfbank_render(wb.h, None, SLOTS + 1, 6, 4, PEAK, 1, None, 0) == -1
            small = np.empty(pic.size - 1, np.uint8)
            assert lib.csdr_wfbank_render(wb.h, lst, n, 6, 4, PEAK, 2, small.ctypes.data_as(C.c_void_p), small.size) == -5
            assert wb.device_view() == ptr
            ctx.synchronize()
            back = np.empty(pic.shape, np.uint8)
            H.check(lib.csdr_dev_download(ctx.h, back.ctypes.data_as(C.c_void_p), C.c_void_p(ptr[0]), back.size))
            assert np.array_equal(back, pic)
        else:                                             # one texel to a half: nothing to filter between (viewport item 1)
            assert lib.csdr_wfbank_render(wb.h, None, SLOTS, 2, 1, PEAK, 1, None, 0) == -1
        # what follows is the twin's: the points of (b) are those of its last good line, not of a refused call
        for b in (wb, twin):
            b.step([(B, None, 1), (A, None, 2)])
            b.update()
            b.step(turns[4])
            b.update()
        same_banks(wb, twin, "after the refusals")
    finally:
        wb.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------ the views
def fed_for_views(ctx, fft_size, waterfalls=False):
    """a bank whose slots stand in the ring states of waterfall_view_cases.ring_states at once: slot 0 in its first turn (row lines - 1 unwritten),
    slot 1 at an offset equal to `lines`, slot 2 across the wrap, slot 3 in the pair layout with one update that crossed the wrap, slot 4 two lines
    in, slot 5 without textures -> (bank, models, [Waterfall] or None)"""
    L = LINES
    wb, models = new_bank(ctx, fft_size)
    wfs = [Waterfall(ctx, fft_size, L, MAX_PENDING) for _ in range(SLOTS)] if waterfalls else None
    rng = np.random.default_rng(4100 + fft_size)

    def lines(n, pair=False):
        a = rng.uniform(-0.2, 1.2, (n, fft_size)).astype(F32)
        a[:, rng.integers(0, fft_size, 3)] = 0.995        # narrow carriers: single bins at the highest index
        return np.stack([np.zeros_like(a), a], axis=2).reshape(n, 2 * fft_size) if pair else a
    calls = [[(s, lines(1), 1) for s in range(5)],
             [(0, lines(3), 3), (1, lines(L - 1), L - 1), (2, lines(L - 1), L - 1), (3, lines(2, True), 2), (4, lines(2), 2)],
             [(2, lines(L - 2), L - 2), (3, lines(9, True), 9)],
             [(2, lines(5), 5)]]
    for call in calls:
        assert wb.step(call) == model_step(models, call)
        wb.update()
        for m in models:
            m.update()
        if wfs:
            for s, a, n in call:
                wfs[s].step(a)
            for s in {it[0] for it in call}:
                wfs[s].update()
    assert models[0].ofs[0] == L - 4 and not models[0].tex[0][L - 1].any()
    assert models[1].ofs[0] == L and models[2].ofs[0] == L - 3 and not models[5].tex_init
    return wb, models, wfs


def widths(half):
    return (2, 3, half, 2 * half, 2 * half + 5)


def heights(lines=LINES):
    return (1, lines - 1, lines, 2 * lines + 1)


SLOT_LISTS = (None, (3, 0, 3, 2, 1), (5, 1, 4, 5, 0, 2, 2))        # all six (the texture-less one among them); a permuted subset with a slot twice; 7 entries
TABLES = (None, "stops256")


def np_atlas(models, table, slots, W, Hh, mode, cols):
    lst = list(range(SLOTS)) if slots is None else list(slots)
    rows = -(-len(lst) // cols)
    out = np.zeros((rows * Hh, cols * W, 4), np.uint8)
    for k, s in enumerate(lst):
        if models[s].tex_init:
            out[(k // cols) * Hh:(k // cols + 1) * Hh, (k % cols) * W:(k % cols + 1) * W] = np_view(models[s], table, W, Hh, mode)
    return out


def view_combos(half):
    """(width, height, slot list, atlas_cols, table): every width with every height; lists, atlas_cols (1, 2, n) and tables in rotation, so that each
    meets every width and every height"""
    out, k = [], 0
    for W in widths(half):
        for Hh in heights():
            slots = SLOT_LISTS[k % 3]
            n = SLOTS if slots is None else len(slots)
            out.append((W, Hh, slots, (1, 2, n)[(k // 3 + k) % 3], TABLES[(k // 2) % 2]))
            k += 1
    # the unaligned-store path by name: a width that is no multiple of 4 beside other tile columns, with an odd count (an unused tile, zero)
    out.append((3, LINES, SLOT_LISTS[1], 2, None))
    out.append((2 * half + 5, 2, SLOT_LISTS[2], 2, "stops256"))
    out.append((2 * half + 5, LINES - 1, SLOT_LISTS[1], 5, None))
    return out


def check_views(ctx, fft_size, mode_name, max_pixels=None):
    """the atlas against np_view tile by tile; max_pixels: skip the combinations whose picture is larger (the emulation runs a thread per work-item)"""
    mode = dict(MODES)[mode_name]
    wb, models, _ = fed_for_views(ctx, fft_size)
    half = fft_size // 2
    n, table_now = 0, None
    try:
        for W, Hh, slots, cols, tab in sorted(view_combos(half), key=lambda c: c[4] is not None):      # (the grey default first: no set_gradient yet)
            lst = SLOTS if slots is None else list(slots)
            count = SLOTS if slots is None else len(slots)
            if max_pixels and -(-count // cols) * cols * W * Hh > max_pixels:
                continue
            if tab != table_now:
                wb.set_gradient(stops256())
                table_now = tab
            table = np_table(stops256()) if tab else np_table()
            got = wb.view(lst, W, Hh, mode_name, cols)
            want = np_atlas(models, table, slots, W, Hh, mode, cols)
            assert got.shape == want.shape and np.array_equal(got, want), (W, Hh, slots, cols, tab, np.argwhere(got != want)[:8])
            n += 1
    finally:
        wb.close()
    return n


def check_view_properties(ctx, fft_size):
    """the grey default; PEAK at width = 2 half, height = lines is the model's unscaled picture; a render that stays on the device; a render leaves
    the textures alone"""
    wb, models, _ = fed_for_views(ctx, fft_size)
    half = fft_size // 2
    try:
        grey = np_table()
        index = [[wb.fetch_index(s, j) for j in range(2)] for s in range(5)]
        got = wb.view(SLOTS, 2 * half, LINES, "peak", 1)
        assert got.shape == (SLOTS * LINES, 2 * half, 4)
        for s in range(SLOTS):
            tile = got[s * LINES:(s + 1) * LINES]
            if models[s].tex_init:
                assert np.array_equal(tile, models[s].rgba(grey, 0, LINES)), s
            else:
                assert not tile.any(), s
        # the default table in LINEAR too, and an unused tile that a larger picture had filled before is zero again
        pic = wb.view([1, 2, 0], 5, 3, "linear", 2)
        assert np.array_equal(pic, np_atlas(models, grey, (1, 2, 0), 5, 3, LINEAR, 2)) and not pic[3:, 5:].any() and pic[3:, :5].any()
        wb.view([1, 2, 0], 5, 3, "linear", 2, fetch=False)
        ptr, w, h = wb.device_view()
        assert (w, h) == (10, 6)
        ctx.synchronize()
        back = np.empty(pic.shape, np.uint8)
        H.check(H.lib().csdr_dev_download(ctx.h, back.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), back.size))
        assert np.array_equal(back, pic)
        for s in range(5):
            for j in range(2):
                assert np.array_equal(wb.fetch_index(s, j), index[s][j])
        # the table outlives a setup; a setup drops the picture
        wb.set_gradient(stops256())
        wb.setup(fft_size, LINES, SLOTS, MAX_PENDING)
        assert H.lib().csdr_wfbank_device_view(wb.h, C.byref(C.c_void_p()), None, None) == -4
        assert not wb.view(SLOTS, 4, 2, "peak", 3).any()                      # no slot has textures now
        line = np.full((1, fft_size), 0.5, F32)
        for _ in range(2):
            wb.step([(1, line, 1)])
            wb.update()
        m = PanelModel(fft_size, LINES)
        for _ in range(2):
            m.set_points(line[0]); m.step(); m.update()
        assert np.array_equal(wb.view([1], 4, 2, "peak", 1), np_view(m, np_table(stops256()), 4, 2, PEAK))
    finally:
        wb.close()


def check_against_waterfalls(ctx, fft_size):
    """six csdr_waterfall objects driven with the same calls: the same textures, offsets and render_view pictures as the bank's slots and tiles --
    over the plan of the life cycle, then over the ring states of the views"""
    wb = WaterfallBank(ctx, fft_size, LINES, SLOTS, MAX_PENDING)
    wfs = [Waterfall(ctx, fft_size, LINES, MAX_PENDING) for _ in range(SLOTS)]

    def compare(where, sizes):
        for s, wf in enumerate(wfs):
            assert wb.lines_buffered(s) == wf.lines_buffered and wb.offset(s, 0) == wf.offset(0) and wb.offset(s, 1) == wf.offset(1), (where, s)
            if wf.offset(0) >= 0:
                for j in range(2):
                    assert np.array_equal(wb.fetch_index(s, j), wf.fetch_index(j)), (where, s, j)
        for W, Hh, name in sizes:
            atlas = wb.view(SLOTS, W, Hh, name, 4)
            for s, wf in enumerate(wfs):
                tile = atlas[(s // 4) * Hh:(s // 4 + 1) * Hh, (s % 4) * W:(s % 4 + 1) * W]
                if wf.offset(0) >= 0:
                    assert np.array_equal(tile, wf.view(W, Hh, name)), (where, s, W, Hh, name)
                else:
                    assert not tile.any(), (where, s)
            assert not atlas[Hh:, 2 * W:].any()           # the two unused tiles
    half = fft_size // 2
    try:
        for k, turn in enumerate(plan(fft_size)):
            taken = wb.step(turn)
            for (s, a, n), t in zip(turn, taken):
                assert (wfs[s].step(None, n_lines=n) if a is None else wfs[s].step(a)) == t, (k, s)
            wb.update()
            for wf in wfs:
                wf.update()
            compare(k, ((7, 5, "linear"), (half + 1, 3, "peak")) if k % 2 else ((2 * half + 5, LINES, "peak"),))
    finally:
        wb.close()
        for wf in wfs:
            wf.close()
    wb, _, wfs = fed_for_views(ctx, fft_size, waterfalls=True)
    try:
        compare("views", [(W, Hh, name) for W in (3, half, 2 * half + 5) for Hh in (1, LINES, 2 * LINES + 1) for name, _ in MODES])
    finally:
        wb.close()
        for wf in wfs:
            wf.close()
