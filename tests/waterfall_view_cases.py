"""The waterfall's viewport (csdr_waterfall_render_view: wf_view_linear / wf_view_peak of kernels_waterfall.hpp, the tap tables of design.hpp) against
a numpy model written for this repository, and the cases that the emulation (tests/test_waterfall_view_emu.py) and the device
(tests/test_gpu_waterfall_view.py) share.  Every comparison is bit for bit; no tolerance appears anywhere.

The model follows include/csdr_hip.h's section "Waterfall viewport" item by item: taps from the integer formulas, LINEAR with every float32
operation rounded on its own, PEAK as a maximum over each pixel's rectangle.  The taps are also pinned against a second, independent statement:
the reference's quad coordinates (src/panel/WaterfallPanel.cpp:185-212) interpolated with fractions.Fraction at the pixel centres."""
import ctypes as C
from fractions import Fraction

import numpy as np

import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import VIEW_TAP, Waterfall
from tests.waterfall_cases import STOPS5, PanelModel, np_table, stops256

F32 = np.float32
LINEAR, PEAK = 0, 1
MODES = (("linear", LINEAR), ("peak", PEAK))


# ------------------------------------------------------------------------------------------------------------------ the taps
def np_columns(fft_size, W, mode):
    half = fft_size // 2
    px = np.arange(W, dtype=np.int64)
    h = 2 * px + 2 > W
    t = np.zeros(W, VIEW_TAP)
    t["half"] = h
    if mode == LINEAR:
        num = np.where(h, 2 * px + 2 - W, 2 * px + 1)
        den = 2 * (W + 1)
        n = (W + 1) + 2 * (half - 2) * num                 # u = 1/2 + (half - 2) num / (W + 1) over 2 (W + 1)
        t["first"], t["count"] = n // den, 2
        t["frac"] = ((n % den).astype(np.float64) / np.float64(den)).astype(F32)
    else:
        n0 = W // 2
        nh = np.where(h, W - n0, n0)
        k = np.where(h, px - n0, px)
        a, b = k * half // nh, (k + 1) * half // nh
        t["first"], t["count"] = a, np.maximum(b - a, 1)
    return t


def np_rows(L, Hh, mode):
    py = np.arange(Hh, dtype=np.int64)
    t = np.zeros(Hh, VIEW_TAP)
    if mode == LINEAR:
        n = L * (2 * py + 1) - Hh
        den = 2 * Hh
        t["first"], t["count"] = n // den, 2               # (numpy's // and % floor, as the header's floor and mod do)
        t["frac"] = ((n % den).astype(np.float64) / np.float64(den)).astype(F32)
    else:
        a, b = py * L // Hh, (py + 1) * L // Hh
        t["first"], t["count"] = a, np.maximum(b - a, 1)
    return t


def _lerp(x, x0, x1, y0, y1):
    return y0 + (y1 - y0) * (x - x0) / (x1 - x0)


def quad_columns(half, W):
    """the reference's two quads: x from -1 to 1 / W with s from 1 / half to 1 - 1 / half, and x from -1 / W to 1 with the same s (:185-186,
    :192-198, :205-211); the pixel centre in normalised device coordinates; the second quad wins strictly inside it -> [(half, i0, alpha)]"""
    out = []
    hp, ht = Fraction(1, W), Fraction(1, half)
    for px in range(W):
        x = Fraction(2 * px + 1, W) - 1
        h = 1 if x > -hp else 0
        s = _lerp(x, -hp, Fraction(1), ht, 1 - ht) if h else _lerp(x, Fraction(-1), hp, ht, 1 - ht)
        u = s * half - Fraction(1, 2)                       # GL_LINEAR: texel centres lie at (i + 1/2) / half
        i0 = u.numerator // u.denominator
        out.append((h, i0, u - i0))
    return out


def quad_rows(L, Hh):
    """t from vofs at the top (y = 1) to 1 + vofs at the bottom (:188, :192-198) without the offset -> [(q, beta)], q relative to waterfall_ofs"""
    out = []
    for py in range(Hh):
        y = 1 - Fraction(2 * py + 1, Hh)                    # row 0 is the top
        t = _lerp(y, Fraction(1), Fraction(-1), Fraction(0), Fraction(1))
        v = t * L - Fraction(1, 2)
        q = v.numerator // v.denominator
        out.append((q, v - q))
    return out


def check_taps_against_the_quads(half, W):
    t = np_columns(2 * half, W, LINEAR)
    q = quad_columns(half, W)
    assert [int(x) for x in t["half"]] == [e[0] for e in q]
    assert [int(x) for x in t["first"]] == [e[1] for e in q]
    assert np.array_equal(t["frac"], np.array([F32(float(e[2].numerator) / float(e[2].denominator)) for e in q], F32))
    assert t["first"].min() >= 0 and t["first"].max() <= half - 2


def check_row_taps_against_the_quads(L, Hh):
    t = np_rows(L, Hh, LINEAR)
    q = quad_rows(L, Hh)
    assert [int(x) for x in t["first"]] == [e[0] for e in q]
    assert np.array_equal(t["frac"], np.array([F32(float(e[1].numerator) / float(e[1].denominator)) for e in q], F32))
    assert t["first"].min() >= -1 and t["first"].max() <= L - 1


# ------------------------------------------------------------------------------------------------------------------ the pictures
def _range_max(a, taps, axis):
    """max of `a` over [first, first + count) along `axis` for every tap: the ranges either partition the axis or are single elements"""
    first, count = taps["first"].astype(np.int64), taps["count"].astype(np.int64)
    if (count == 1).all():
        return np.take(a, first, axis=axis)
    assert first[0] == 0 and (first[1:] == first[:-1] + count[:-1]).all() and first[-1] + count[-1] == a.shape[axis]
    return np.maximum.reduceat(a, first, axis=axis)


def np_view(m, table, W, Hh, mode):
    """the W x Hh view of PanelModel m -> [Hh, W, 4] uint8"""
    L, half, ofs = m.lines, m.half, m.ofs[0]
    ct, rt = np_columns(m.fft_size, W, mode), np_rows(L, Hh, mode)
    hh = ct["half"].astype(np.int64)
    if mode == PEAK:
        scrolled = (ofs + np.arange(L)) % L
        n0 = W // 2
        parts = [_range_max(_range_max(m.tex[h][scrolled], rt, 0), ct[:n0] if h == 0 else ct[n0:], 1) for h in range(2)]
        assert not hh[:n0].any() and hh[n0:].all()
        return table[np.concatenate(parts, axis=1)]
    both = np.stack(m.tex)
    i0 = ct["first"].astype(np.int64)[None, :]
    j0 = (ofs + rt["first"].astype(np.int64) + L) % L
    j1 = (j0 + 1) % L

    def colour(j, i):
        return table[both[hh[None, :], j[:, None], i]][..., :3].astype(F32)
    c00, c10, c01, c11 = colour(j0, i0), colour(j0, i0 + 1), colour(j1, i0), colour(j1, i0 + 1)
    al, be = ct["frac"][None, :, None], rt["frac"][:, None, None]
    top = c00 + al * (c10 - c00)                            # float32 arrays: every operation is rounded on its own
    bot = c01 + al * (c11 - c01)
    mm = top + be * (bot - top)
    assert top.dtype == F32 and mm.dtype == F32
    out = np.empty((Hh, W, 4), np.uint8)
    out[..., :3] = (mm + F32(0.5)).astype(np.uint8)
    out[..., 3] = 255
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases
FFT_SIZES = (16, 30, 601, 2048)
LINES = (7, 12)


def widths(half):
    return (2, 3, 16, 17, 2 * half, 2 * half + 1, 5 * half)


def heights(lines):
    return (1, 3, lines - 2, lines, 2 * lines + 1)


class Fed:
    """a waterfall and the model, fed the same lines"""

    def __init__(self, ctx, fft_size, lines, seed):
        self.rng = np.random.default_rng(seed)
        self.wf = Waterfall(ctx, fft_size, lines, max_pending=32)
        self.m = PanelModel(fft_size, lines)

    def feed(self, n):
        a = self.rng.uniform(-0.2, 1.2, (n, self.m.fft_size)).astype(F32)
        a[:, self.rng.integers(0, self.m.fft_size, 3)] = 0.995      # narrow carriers: single bins at the highest index
        for row in a:
            self.m.set_points(row)
            self.m.step()
        self.wf.step(a)
        self.wf.update(); self.m.update()


def ring_states(f):
    """the three ring states of the issue, with a table each; yields (name, table)"""
    L = f.m.lines
    f.feed(1)                                              # dropped; creates the textures
    f.feed(3)
    assert f.wf.offset(0) == L - 4 < L - 1 and not f.m.tex[0][L - 1].any()
    yield "first turn", np_table()
    f.feed(L - 4)
    assert f.wf.offset(0) == L == f.m.ofs[0]
    f.wf.set_gradient(STOPS5)
    yield "ofs == lines", np_table(STOPS5)
    f.feed(L - 2)
    f.feed(5)                                              # two rows below the wrap, three above it
    assert f.wf.offset(0) == L - 3
    f.wf.set_gradient(stops256())
    yield "across the wrap", np_table(stops256())


def check_views(ctx, fft_size, lines):
    f = Fed(ctx, fft_size, lines, 4000 + fft_size + lines)
    half = fft_size // 2
    n = 0
    try:
        for state, table in ring_states(f):
            # the ring's state bears on the rows alone: every height in every state, every width in the last one (all rows written, ofs inside)
            for W in (widths(half) if state == "across the wrap" else (17, 2 * half + 1)):
                for Hh in heights(lines):
                    for name, mode in MODES:
                        got = f.wf.view(W, Hh, name)
                        want = np_view(f.m, table, W, Hh, mode)
                        assert got.shape == want.shape and np.array_equal(got, want), (state, W, Hh, name, np.argwhere(got != want)[:8])
                        n += 1
    finally:
        f.wf.close()
    return n


def _download(ctx, ptr, shape):
    back = np.empty(shape, np.uint8)
    H.check(H.lib().csdr_dev_download(ctx.h, back.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), back.size))
    return back


def check_view_properties(ctx, fft_size, lines):
    """PEAK at texture resolution is fetch_rgba; LINEAR at H = lines reads the ring rows of fetch_rgba; a view leaves the object's other results
    alone; the refusals change nothing"""
    f = Fed(ctx, fft_size, lines, 5000 + fft_size + lines)
    half = fft_size // 2
    lib = H.lib()
    try:
        # before the textures exist: what fetch_rgba answers in that state
        rc = lib.csdr_waterfall_fetch_rgba(f.wf.h, 0, 1, None, 0)
        assert rc == -4 and lib.csdr_waterfall_render_view(f.wf.h, 16, 3, PEAK, None, 0) == rc
        assert lib.csdr_waterfall_device_view(f.wf.h, C.byref(C.c_void_p()), None, None) == -4
        for state, table in ring_states(f):
            whole = f.wf.fetch_rgba(0, lines)
            assert np.array_equal(f.wf.view(2 * half, lines, "peak"), whole), state
            for W in (2, 17, 2 * half + 1):
                ct = np_columns(fft_size, W, LINEAR)
                at = ct["half"].astype(np.int64) * half + ct["first"]
                a, b = whole[:, at, :3].astype(F32), whole[:, at + 1, :3].astype(F32)
                want = np.full((lines, W, 4), 255, np.uint8)
                want[..., :3] = ((a + ct["frac"][None, :, None] * (b - a)) + F32(0.5)).astype(np.uint8)
                assert np.array_equal(f.wf.view(W, lines, "linear"), want), (state, W)
        # a view between a fetch_rgba that stays on the device and its pointer: the picture, the pointer and the textures are those of before
        table = np_table(stops256())
        index = [f.wf.fetch_index(j) for j in range(2)]
        part = f.wf.fetch_rgba(2, 4)
        f.wf.fetch_rgba(2, 4, fetch=False)
        ptr = f.wf.device_rgba()
        pic = f.wf.view(17, 5, "linear")
        f.wf.view(16, 3, "peak", fetch=False)
        vptr, vw, vh = f.wf.device_view()
        assert (vw, vh) == (16, 3) and vptr != ptr
        assert f.wf.device_rgba() == ptr
        ctx.synchronize()
        assert np.array_equal(_download(ctx, ptr, part.shape), part)
        kept = _download(ctx, vptr, (3, 16, 4))
        assert np.array_equal(kept, np_view(f.m, table, 16, 3, PEAK))
        assert np.array_equal(f.wf.fetch_rgba(2, 4), part)
        for j in range(2):
            assert np.array_equal(f.wf.fetch_index(j), index[j])
        # the refusals
        buf = np.empty(16 * 3 * 4 - 1, np.uint8)
        for W, Hh, mode, rc in ((1, 3, PEAK, -1), (16385, 3, LINEAR, -1), (16, 0, PEAK, -1), (16, 16385, LINEAR, -1), (16, 3, 2, -1), (16, 3, -1, -1)):
            assert lib.csdr_waterfall_render_view(f.wf.h, W, Hh, mode, None, 0) == rc, (W, Hh, mode)
        assert lib.csdr_waterfall_render_view(f.wf.h, 16, 3, LINEAR, buf.ctypes.data_as(C.c_void_p), buf.size) == -5
        assert f.wf.device_view() == (vptr, 16, 3)
        ctx.synchronize()
        assert np.array_equal(_download(ctx, vptr, (3, 16, 4)), kept)
        assert np.array_equal(f.wf.view(17, 5, "linear"), pic)
        for j in range(2):
            assert np.array_equal(f.wf.fetch_index(j), index[j])
        # a ring of fft_size 2 has one texel per half: nothing to filter between
        f.wf.setup(2, lines, 32)
        f.wf.step(None); f.wf.update()
        assert f.wf.fetch_rgba(0, 1).shape == (1, 2, 4)
        assert lib.csdr_waterfall_render_view(f.wf.h, 2, 1, PEAK, None, 0) == -1
        assert lib.csdr_waterfall_device_view(f.wf.h, C.byref(C.c_void_p()), None, None) == -4      # a setup drops the view
    finally:
        f.wf.close()


def check_wide_footprints(ctx, fft_size=131075, lines=3):
    """a pixel wider than a workgroup's LDS slots (16 KB): fft_size 131075 has 65537 texels to a half, which 2, 3 and 5 pixels share out as 65537,
    32768 and 21845 apiece -- folded -- and 9 pixels as 16384 and 13107 -- whole, one pixel to a tile.  PEAK against the model; LINEAR once."""
    f = Fed(ctx, fft_size, lines, 6000)
    try:
        f.feed(1)
        f.feed(2)
        f.feed(2)                                          # ofs: 2 -> 0 -> 3, then 1
        assert f.wf.offset(0) == 1
        f.wf.set_gradient(STOPS5)
        table = np_table(STOPS5)
        for W in (2, 3, 5, 9):
            for Hh in (1, 3, 7):
                got = f.wf.view(W, Hh, "peak")
                want = np_view(f.m, table, W, Hh, PEAK)
                assert np.array_equal(got, want), (W, Hh, np.argwhere(got != want)[:8])
        # every pixel's maximum is the carrier's index, and the carriers are three bins of 131075: LINEAR at the same size shows none of them
        assert (f.wf.view(5, 3, "peak")[..., :3] == table[252, :3]).all()
        got = f.wf.view(5, 3, "linear")
        assert np.array_equal(got, np_view(f.m, table, 5, 3, LINEAR)) and not (got[..., :3] == table[252, :3]).all()
    finally:
        f.wf.close()
