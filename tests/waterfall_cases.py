"""The waterfall raster (csdr_waterfall: kernels_waterfall.hpp, csdr_waterfall.hip) against a restatement of WaterfallPanel and Gradient written for
this repository in numpy -- the model below -- and the cases that the emulation (tests/test_waterfall_emu.py) and the device
(tests/test_gpu_waterfall.py) share.  Every comparison is bit for bit; no tolerance appears anywhere.

The model follows include/csdr_hip.h's section on the waterfall item by item (quantiser in float64, the panel's setPoints / step / update with its
runs, Gradient::generate with every float32 operation rounded on its own, the picture under GL_REPEAT)."""
import ctypes as C

import numpy as np

import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import SpectrumProcessor, Waterfall, design_gradient

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ the model
def np_quantise(v):
    """wv = v < 0 ? 0 : (v > 0.99 ? 0.99 : v) stored to a float (the comparison with 0.99 in double), then (unsigned char)floor(wv * 255.0) in
    double; NaN -> 0 (the library's own definition)"""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        wv = np.where(v < 0, F32(0), np.where(v.astype(np.float64) > 0.99, F32(0.99), v)).astype(F32)
        wv = np.where(np.isnan(v), F32(0), wv)
        return np.floor(wv.astype(np.float64) * 255.0).astype(np.uint8)


class PanelModel:
    """WaterfallPanel's state machine, restated: setup, setPoints, step, update"""

    def __init__(self, fft_size, lines):
        self.points = np.zeros(0, F32)
        self.setup(fft_size, lines)

    def setup(self, fft_size, lines):
        self.fft_size, self.half, self.lines = fft_size, fft_size // 2, lines
        self.lines_buffered = 0
        p = np.zeros(fft_size, F32)
        n = min(fft_size, self.points.size)
        p[:n] = self.points[:n]
        self.points = p
        self.tex_init = self.buffer_init = False
        self.pending = [[], []]
        self.tex = None
        self.ofs = None

    def set_points(self, pts):
        pts = np.asarray(pts, F32).reshape(-1)
        if pts.size == 2 * self.fft_size:
            self.points = pts[1::2].copy()
        elif pts.size == self.fft_size:
            self.points = pts.copy()
        # any other length: the previous points stay

    def step(self):
        self.buffer_init = True
        if not self.tex_init:
            return 0
        q = np_quantise(self.points)
        for j in range(2):
            self.pending[j].append(q[j * self.half:(j + 1) * self.half])
        self.lines_buffered += 1
        return 1

    def update(self):
        if not self.buffer_init:
            return
        if not self.tex_init:
            self.tex = [np.zeros((self.lines, self.half), np.uint8) for _ in range(2)]
            self.ofs = [self.lines - 1, self.lines - 1]
            self.tex_init = True
        rev = [list(reversed(self.pending[j])) for j in range(2)]
        run_ofs = 0
        while self.lines_buffered:
            run = min(self.lines_buffered, self.ofs[0])
            for j in range(2):
                for t in range(run):
                    self.tex[j][self.ofs[j] - run + t] = rev[j][run_ofs + t]
                self.ofs[j] -= run
                if self.ofs[j] == 0:
                    self.ofs[j] = self.lines
            run_ofs += run
            self.lines_buffered -= run
        self.pending = [[], []]

    def rgba(self, table, first_row, n_rows):
        rows = (self.ofs[0] + first_row + np.arange(n_rows)) % self.lines
        idx = np.concatenate([self.tex[0][rows], self.tex[1][rows]], axis=1)
        return table[idx]


def np_gradient(stops, length):
    """Gradient::generate(length): (length, 3) float32"""
    stops = np.asarray(stops, F32).reshape(-1, 3)
    n = stops.shape[0]
    chunk = length // (n - 1)
    out = np.zeros((length, 3), F32)
    p = 0
    for j in range(n - 1):
        if chunk * (n - 1) < length and j == n - 2:
            chunk += length - chunk * (n - 1)
        idx = (np.arange(chunk).astype(F32) / F32(chunk)).astype(F32)
        c1, c2 = stops[j], stops[j + 1]
        d = (c2 - c1).astype(F32)
        m = (d[None, :] * idx[:, None]).astype(F32)
        c = (c1[None, :] + m).astype(F32)
        c = np.where(c < 0, F32(0), c)
        c = np.where(c > 1, F32(1), c)
        out[p:p + chunk] = c
        p += chunk
    assert p == length
    return out


def np_table(stops=None):
    """the 256 x RGBA8 table: (uint8)(c * 255.0f + 0.5f), alpha 255; no stops: the grey ramp"""
    t = np.empty((256, 4), np.uint8)
    t[:, 3] = 255
    if stops is None:
        t[:, :3] = np.arange(256, dtype=np.uint8)[:, None]
        return t
    g = np_gradient(stops, 256)
    t[:, :3] = ((g * F32(255.0)).astype(F32) + F32(0.5)).astype(F32).astype(np.uint8)
    return t


# ------------------------------------------------------------------------------------------------------------------ helpers
def quantise_through_panel(ctx, values, fft_size, pair, device=False):
    """`values` (float32, any count) as lines of fft_size points through setup / step / update / fetch_index -> the bytes of the points that are
    drawn, line by line, and the values they belong to.  With device=True `values` is a CUDA tensor and so is what goes into step."""
    n_lines = -(-int(values.shape[0]) // fft_size)
    half = fft_size // 2
    wf = Waterfall(ctx, fft_size, n_lines + 2, max_pending=n_lines)
    try:
        assert wf.step(None) == 0                       # dropped: no textures yet
        wf.update()
        assert wf.offset(0) == n_lines + 1 and wf.offset(1) == n_lines + 1
        if device:
            import torch
            lines = torch.zeros(n_lines * fft_size, dtype=torch.float32, device=values.device)
            lines[:values.shape[0]] = values
            lines = lines.reshape(n_lines, fft_size)
            if pair:
                lines = torch.stack([torch.full_like(lines, 7.0), lines], dim=2).reshape(n_lines, 2 * fft_size)
        else:
            lines = np.zeros(n_lines * fft_size, F32)
            lines[:values.shape[0]] = values
            lines = lines.reshape(n_lines, fft_size)
            if pair:
                lines = np.stack([np.full_like(lines, 7.0), lines], axis=2).reshape(n_lines, 2 * fft_size)
        if device:
            torch.cuda.synchronize()                    # (the tensor was made on torch's stream, the waterfall works on its own)
        assert wf.step(lines) == n_lines
        assert wf.lines_buffered == n_lines
        wf.update()
        assert wf.lines_buffered == 0 and wf.offset(0) == 1
        got = np.concatenate([wf.fetch_index(0)[1:n_lines + 1][::-1], wf.fetch_index(1)[1:n_lines + 1][::-1]], axis=1)      # newest line first in the ring
        assert not wf.fetch_index(0)[0].any() and not wf.fetch_index(0)[n_lines + 1].any()
    finally:
        wf.close()
    return got, n_lines, half


def drawn(values, fft_size):
    """the values of `values` laid out in lines of fft_size that the panel draws (2 * half per line)"""
    n_lines = -(-values.size // fft_size)
    lines = np.zeros(n_lines * fft_size, F32)
    lines[:values.size] = values
    return lines.reshape(n_lines, fft_size)[:, :2 * (fft_size // 2)]


def special_values():
    v = []
    for k in range(256):
        x = F32(k) / F32(255)
        xs = [x]
        lo = hi = x
        for _ in range(4):
            lo = np.nextafter(lo, F32(-1), dtype=F32)
            hi = np.nextafter(hi, F32(2), dtype=F32)
            xs += [lo, hi]
        v += xs
        y = F32(np.float64(k) / 255.0)                   # the correctly rounded quotient too
        v += [y, np.nextafter(y, F32(-1), dtype=F32), np.nextafter(y, F32(2), dtype=F32)]
    c = F32(0.99)
    v += [c, np.nextafter(c, F32(0), dtype=F32), np.nextafter(c, F32(2), dtype=F32), F32(np.nextafter(np.float64(0.99), 0)), F32(1), F32(5), F32(np.inf),
          F32(-np.inf), F32(0.0), F32(-0.0), F32(-1e-45), F32(-1e-40), F32(1e-45), F32(1e-40), F32(np.nan), F32(-1.0), F32(3.4e38), F32(-3.4e38),
          F32(2.0 ** -9), np.nextafter(F32(2.0 ** -9), F32(0), dtype=F32), F32(1.0 / 255.0)]
    return np.array(v, F32)


# ------------------------------------------------------------------------------------------------------------------ the cases
FFT_SIZES = (2, 16, 30, 601, 2048)


def check_quantiser_specials(ctx, fft_size, pair):
    v = special_values()
    rng = np.random.default_rng(fft_size)
    v = np.concatenate([v, rng.uniform(-0.2, 1.2, 3 * fft_size + 5).astype(F32)])
    got, n_lines, half = quantise_through_panel(ctx, v, fft_size, pair)
    want = np_quantise(drawn(v, fft_size))
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert want.max() == 252
    return v.size


def check_quantiser_binade(ctx, exponent, fft_size=65536):
    """every float32 of [2^exponent, 2^(exponent + 1))"""
    bits = (np.arange(1 << 23, dtype=np.uint32) + np.uint32((exponent + 127) << 23))
    v = bits.view(F32)
    got, n_lines, half = quantise_through_panel(ctx, v, fft_size, False)
    want = np_quantise(drawn(v, fft_size))
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    return v.size


def _rc_step(wf, lines_arr):
    a = np.ascontiguousarray(lines_arr, F32)
    taken = C.c_int(-7)
    rc = H.lib().csdr_waterfall_step(wf.h, a.ctypes.data_as(C.c_void_p), 0, int(a.shape[-1]), int(a.shape[0]), C.byref(taken))
    return rc, taken.value


def _same_state(wf, m):
    assert wf.lines_buffered == m.lines_buffered
    if m.tex_init:
        assert wf.offset(0) == m.ofs[0] and wf.offset(1) == m.ofs[1]
        for j in range(2):
            got = wf.fetch_index(j)
            assert np.array_equal(got, m.tex[j]), (j, np.argwhere(got != m.tex[j])[:8])
    else:
        assert wf.offset(0) == -1


LIFE_COUNTS = (3, 5, 7, 1, 20)


def check_life_cycle(ctx, fft_size, pair=False, lines=7):
    """lines = 7; 2 steps before the first update (dropped), then 3, 5 (the worked example of csdr_hip.h), 7, 1 and 20 lines between updates with
    max_pending 32; textures, offsets and lines_buffered after every update; the CSDR_ERANGE refusal; a repeated line after a wrong-length input"""
    rng = np.random.default_rng(1000 + fft_size)
    wf = Waterfall(ctx, fft_size, lines, max_pending=32)
    m = PanelModel(fft_size, lines)

    def feed(n):
        a = rng.uniform(-0.2, 1.2, (n, fft_size)).astype(F32)
        if pair:
            a = np.stack([rng.uniform(0, 1, a.shape).astype(F32), a], axis=2).reshape(n, 2 * fft_size)
        want = 0
        for row in a:
            m.set_points(row)
            want += m.step()
        assert wf.step(a) == want
    try:
        wf.update()                                       # before any step: nothing happens (no textures)
        m.update()
        _same_state(wf, m)
        feed(2)                                           # dropped
        assert wf.lines_buffered == 0
        wf.update(); m.update()
        _same_state(wf, m)
        assert wf.offset(0) == lines - 1 and not wf.fetch_index(0).any()
        # the points of the dropped steps were kept all the same: a step without points repeats the last of them
        assert wf.step(None) == 1 and m.step() == 1
        wf.update(); m.update()
        _same_state(wf, m)
        for k, n in enumerate(LIFE_COUNTS):
            feed(n)
            if k == 2:                                    # a line of the wrong length: the previous points are stepped again
                assert wf.step(np.full(5 if fft_size != 5 else 6, 0.5, F32)) == 1
                m.set_points(np.full(5 if fft_size != 5 else 6, 0.5, F32))
                m.step()
                assert wf.step(None, n_lines=2) == 2
                m.step(); m.step()
            assert wf.lines_buffered == m.lines_buffered
            wf.update(); m.update()
            _same_state(wf, m)
        if lines == 7:
            assert m.ofs[0] == wf.offset(0)
        # the refusal: 30 lines wait, 3 more would exceed max_pending = 32 -- nothing is taken, nothing changes
        feed(30)
        rc, taken = _rc_step(wf, rng.uniform(0, 1, (3, fft_size)).astype(F32))
        assert rc == -5 and taken == 0 and wf.lines_buffered == 30
        rc, taken = _rc_step(wf, np.zeros((3, 5), F32))                      # (a repeat is refused alike)
        assert rc == -5 and taken == 0 and wf.lines_buffered == 30
        assert wf.step(None, n_lines=2) == 2                                  # the points are those of line 30, not of the refused call
        m.step(); m.step()
        wf.update(); m.update()
        _same_state(wf, m)
        # a new setup: lines_buffered cleared, textures gone until the next update, which zero-fills them
        feed(4)
        wf.setup(fft_size, lines + 2, 32)
        m.setup(fft_size, lines + 2)
        _same_state(wf, m)
        feed(1)
        wf.update(); m.update()
        feed(3)
        wf.update(); m.update()
        _same_state(wf, m)
    finally:
        wf.close()
    return m


def check_worked_example(ctx, fft_size=16):
    """the example of csdr_hip.h: lines = 7; A, B, C -> rows 3, 4, 5 = C, B, A, ofs 3; D .. H -> rows 0 .. 6 = H, G, F, C, B, E, D, ofs 5"""
    wf = Waterfall(ctx, fft_size, 7, max_pending=8)
    try:
        wf.step(None); wf.update()
        val = {c: F32((i + 1) * 10 / 255.0 + 0.001) for i, c in enumerate("ABCDEFGH")}
        byte = {c: int(np_quantise(np.array([val[c]]))[0]) for c in val}
        assert len(set(byte.values())) == 8 and 0 not in byte.values()
        wf.step(np.stack([np.full(fft_size, val[c], F32) for c in "ABC"])); wf.update()
        assert wf.offset(0) == 3 and wf.offset(1) == 3
        for j in range(2):
            assert [int(r[0]) for r in wf.fetch_index(j)] == [0, 0, 0, byte["C"], byte["B"], byte["A"], 0]
        wf.step(np.stack([np.full(fft_size, val[c], F32) for c in "DEFGH"])); wf.update()
        assert wf.offset(0) == 5
        for j in range(2):
            t = wf.fetch_index(j)
            assert [int(r[0]) for r in t] == [byte[c] for c in "HGFCBED"]
            assert (t == t[:, :1]).all()
    finally:
        wf.close()


STOPS5 = [[0.0, 0.0, 0.1], [0.0, 0.2, 1.3], [-0.2, 1.0, 0.0], [1.0, 0.5, 0.25], [1.0, 1.0, 1.0]]


def stops256():
    rng = np.random.default_rng(256)
    return rng.uniform(-0.1, 1.1, (256, 3)).astype(F32)


def check_rgba(ctx, fft_size):
    """grey default, a five-stop and a 256-stop gradient; windows that cross the wrap; an offset equal to `lines`"""
    lines = 7
    rng = np.random.default_rng(77 + fft_size)
    wf = Waterfall(ctx, fft_size, lines, max_pending=32)
    m = PanelModel(fft_size, lines)

    def feed(n):
        a = rng.uniform(-0.2, 1.2, (n, fft_size)).astype(F32)
        for row in a:
            m.set_points(row)
            m.step()
        wf.step(a)
        wf.update(); m.update()

    def pictures(table):
        for first, n in ((0, lines), (3, 4), (lines - 1, 1), (2, 1), (0, 1), (1, lines - 1)):
            got = wf.fetch_rgba(first, n)
            want = m.rgba(table, first, n)
            assert got.shape == want.shape and np.array_equal(got, want), (first, n, np.argwhere(got != want)[:8])
    try:
        feed(1)                                           # dropped; creates the textures
        feed(6)                                           # rows 0 .. 5, offset 6 -> 0 -> lines
        assert wf.offset(0) == lines == m.ofs[0]
        pictures(np_table())
        feed(9)                                           # crosses the wrap inside one update
        assert 0 < wf.offset(0) < lines
        pictures(np_table())
        wf.set_gradient(STOPS5)
        pictures(np_table(STOPS5))
        feed(2)
        wf.set_gradient(stops256())
        pictures(np_table(stops256()))
        wf.fetch_rgba(0, lines, fetch=False)
        assert wf.device_rgba()
        # refusals
        lib = H.lib()
        buf = np.empty(16, np.uint8)
        assert lib.csdr_waterfall_fetch_rgba(wf.h, 0, lines + 1, None, 0) == -1
        assert lib.csdr_waterfall_fetch_rgba(wf.h, 3, lines - 2, None, 0) == -1
        assert lib.csdr_waterfall_fetch_rgba(wf.h, 0, lines, buf.ctypes.data_as(C.c_void_p), buf.size) == -5
        bad = np.zeros((258, 3), F32)
        assert lib.csdr_waterfall_set_gradient(wf.h, bad.ctypes.data_as(C.c_void_p), 258) == -1
        assert lib.csdr_waterfall_set_gradient(wf.h, bad.ctypes.data_as(C.c_void_p), 1) == -1
        pictures(np_table(stops256()))                    # a refused gradient leaves the table alone
    finally:
        wf.close()


def noise(n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.05
    x += 0.5 * np.exp(2j * np.pi * 0.123 * np.arange(n)) + 0.3                  # a carrier and a DC spike
    return x.astype(np.complex64)


def check_step_spec(ctx, fft_size, hide_dc, bandwidth=None, frames=3):
    """`frames` contiguous frames of a spectrum: the bytes equal the model's quantiser applied to what csdr_spec_fetch returns for the same frames, and
    csdr_spec_fetch gives the same floats before and after the step"""
    fs, center = 2400000, 100000000
    sp = SpectrumProcessor(ctx, fft_size, max_frames=frames)
    wf = Waterfall(ctx, fft_size, frames + 3, max_pending=frames)
    try:
        sp.set_hide_dc(hide_dc, center_freq=center, bandwidth=bandwidth or fs, input_freq=center)
        x = noise(frames * 2 * fft_size, fft_size)
        assert sp.process(x, 1, x.size, contiguous=True) == frames
        before = [sp.fetch(f)[0] for f in range(frames)]
        if hide_dc:                                       # the overwrite did change something in what the fetch returns
            sp.set_hide_dc(False)
            assert any(not np.array_equal(sp.fetch(f)[0], before[f]) for f in range(frames))
            sp.set_hide_dc(True)
        assert wf.step_spec(sp, 0, frames) == 0           # no textures yet: dropped
        wf.update()
        assert wf.step_spec(sp, 1, frames - 1) == frames - 1
        assert wf.step_spec(sp, 0, 1) == 1
        wf.update()
        after = [sp.fetch(f)[0] for f in range(frames)]
        for a, b in zip(before, after):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        half = fft_size // 2
        order = list(range(1, frames)) + [0]              # the order the lines were stepped in; the newest sits at the lowest row
        n = frames
        ofs = wf.offset(0)
        assert ofs == frames + 2 - n
        for j in range(2):
            t = wf.fetch_index(j)
            for k, f in enumerate(reversed(order)):
                want = np_quantise(before[f][1::2])[j * half:(j + 1) * half]
                assert np.array_equal(t[ofs + k], want), (j, f, np.argwhere(t[ofs + k] != want)[:8])
        assert len({bytes(np_quantise(b[1::2])) for b in before}) > 1 or frames == 1
        # frames outside the last process are refused; a spectrum of another size steps the previous points
        assert H.lib().csdr_waterfall_step_spec(wf.h, sp.h, 1, frames, None) == -1
    finally:
        wf.close()
        sp.close()


def check_design_gradient(n_colors, length=256, seed=0):
    rng = np.random.default_rng(seed + n_colors)
    stops = rng.uniform(-0.3, 1.3, (n_colors, 3)).astype(F32)       # stops outside [0, 1] too
    r, g, b = design_gradient(stops, length)
    want = np_gradient(stops, length)
    for got, k in ((r, 0), (g, 1), (b, 2)):
        assert np.array_equal(got.view(np.uint32), want[:, k].view(np.uint32)), (n_colors, k, np.argwhere(got != want[:, k])[:8])
    return want
