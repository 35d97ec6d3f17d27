"""The shared cases of the overlay bank (csdr_overlay; include/csdr_hip.h, "Overlay bank") against tests/overlay_oracle.py, byte for byte: the
smallest shapes at which the rule or the kernel can go wrong.  Run by the emulation (tests/test_overlay_emu.py), on the device
(tests/test_gpu_overlay.py) and by the host mirror (tests/test_overlay_host.py).  The font is synthetic and made here: a seeded random 64 x 32
coverage plane and a glyph table with zero-width glyphs, negative offsets and one glyph in the far corner of the plane."""
import ctypes as C

import numpy as np

from tests import overlay_oracle as O

FONT_W, FONT_H, LINE_HEIGHT = 64, 32, 9
FONT = np.random.default_rng(7).integers(0, 256, (FONT_H, FONT_W), dtype=np.uint8)
FONT[0, 0], FONT[1, 1], FONT[31, 63] = 0, 255, 255


def _glyphs():
    """id, x, y, w, h, xoffset, yoffset, xadvance: the characters the planners' labels use and a few odd ones"""
    r = np.random.default_rng(8)
    g = []
    for k, ch in enumerate("0123456789.-dB[]VRMS"):
        w, h = int(r.integers(2, 7)), int(r.integers(3, 9))
        g.append((ord(ch), int(r.integers(0, FONT_W - w)), int(r.integers(0, FONT_H - h)), w, h, int(r.integers(-2, 3)), int(r.integers(-3, 3)), int(r.integers(3, 8))))
    g.append((ord(" "), 0, 0, 0, 0, 0, 0, 4))                       # no picture, an advance
    g.append((ord("_"), 5, 5, 0, 3, 1, 1, 0))                       # zero width, zero advance
    g.append((ord("#"), FONT_W - 6, FONT_H - 7, 6, 7, -3, -2, 5))   # the far corner of the plane, negative offsets
    g.append((ord("0"), 0, 0, 1, 1, 0, 0, 1))                       # a second '0': the first match is taken
    return [dict(zip(("id", "x", "y", "w", "h", "xoffset", "yoffset", "xadvance"), t)) for t in g]


GLYPHS = _glyphs()


def glyph_array():
    from cubicsdr_amd.engine import GLYPH_DTYPE
    return np.array([tuple(g[k] for k in GLYPH_DTYPE.names) for g in GLYPHS], GLYPH_DTYPE)


def _random_prims(r, n, W, Hh, masked=True):
    """rectangles around and across the tile, every mode, a third of them glyph windows"""
    out = []
    for _ in range(n):
        w, h = int(r.integers(0, W + 6)), int(r.integers(0, Hh + 6))
        x, y = int(r.integers(-w - 2, W + 3)), int(r.integers(-h - 2, Hh + 3))
        rgba = tuple(int(v) for v in r.integers(0, 256, 4))
        mode = int(r.integers(0, 3))
        if masked and r.integers(0, 3) == 0:
            w, h = min(w, FONT_W), min(h, FONT_H)
            out.append((x, y, w, h, rgba, mode, int(r.integers(0, FONT_W - w + 1)), int(r.integers(0, FONT_H - h + 1))))
        else:
            out.append((x, y, w, h, rgba, mode, -1, 0))
    return out


def _cases():
    c = {}
    r = np.random.default_rng(3)

    def base_for(W, Hh, n, cols):
        return r.integers(1, 256, (-(-n // cols) * Hh, cols * W, 4), dtype=np.uint8)
    # one pixel: every mode on it, in order
    c["w1_h1"] = dict(prims=[(0, 0, 1, 1, (200, 100, 50, 128), O.OVER), (0, 0, 1, 1, (90, 200, 10, 77), O.ADD), (-3, -3, 9, 9, (1, 2, 3, 255), O.OVER, 2, 3),
                             (0, 0, 1, 1, (250, 250, 250, 200), O.ADD)], runs=[(0, 4)], W=1, H=1, base="host")
    c["w1_h1_copy"] = dict(prims=[(0, 0, 1, 1, (9, 8, 7, 66), O.COPY)], runs=[(0, 1)], W=1, H=1, base=None)
    # five tiles, three to a row: the sixth is unused and must be zero over a non-zero base; an empty list; a shared run; overlapping runs
    p7 = _random_prims(r, 12, 7, 5)
    c["atlas_w7_h5"] = dict(prims=p7, runs=[(0, 5), (0, 0), (0, 5), (3, 9), (12, 0)], W=7, H=5, cols=3, base="host")
    c["atlas_w7_h5_no_base"] = dict(c["atlas_w7_h5"], base=None)
    c["w7_h1"] = dict(prims=_random_prims(r, 8, 7, 1), runs=[(0, 8), (2, 6)], W=7, H=1, cols=2, base="host")
    # one column block, three row groups of which the last holds one row; the picture rows keep the 16-byte grid
    c["w64_h33"] = dict(prims=_random_prims(r, 40, 64, 33), runs=[(0, 40)], W=64, H=33, base="host")
    # edges, one by one
    W, Hh = 64, 33
    edges = [(-5, 3, 10, 4, (255, 0, 0, 128), O.OVER), (W - 5, 3, 10, 4, (0, 255, 0, 128), O.OVER), (10, -3, 6, 7, (0, 0, 255, 128), O.OVER),
             (10, Hh - 3, 6, 7, (255, 255, 0, 128), O.OVER), (-4, -4, W + 8, Hh + 8, (7, 7, 7, 40), O.ADD),
             (-20, 5, 10, 5, (1, 1, 1, 255), O.COPY), (W, 5, 10, 5, (1, 1, 1, 255), O.COPY), (5, -9, 5, 9, (1, 1, 1, 255), O.COPY), (5, Hh, 5, 9, (1, 1, 1, 255), O.COPY),
             (1 << 20, 1 << 20, 5, 5, (1, 1, 1, 255), O.COPY), (-(1 << 20), -(1 << 20), 5, 5, (1, 1, 1, 255), O.COPY), (-(1 << 20), 0, 2147483647, 3, (0, 30, 0, 255), O.ADD),
             (20, 10, 0, 5, (9, 9, 9, 255), O.COPY), (20, 10, 5, 0, (9, 9, 9, 255), O.COPY),
             (30, 10, 8, 8, (255, 255, 255, 0), O.OVER), (30, 10, 8, 8, (255, 255, 255, 0), O.ADD), (40, 10, 8, 8, (12, 34, 56, 255), O.OVER),
             (30, 20, 20, 6, (200, 200, 200, 255), O.ADD), (30, 20, 20, 6, (200, 200, 200, 255), O.ADD),          # saturates
             (2, 20, 12, 9, (10, 200, 30, 180), O.COPY, 7, 11),                                                  # COPY under a mask
             (-4, -3, 9, 8, (255, 255, 255, 255), O.OVER, 20, 5), (W - 3, Hh - 2, 6, 7, (0, 0, 0, 255), O.OVER, FONT_W - 6, FONT_H - 7),   # negative origin; far corner
             (50, -2, 14, 8, (90, 0, 200, 200), O.ADD, 0, 0)]
    c["edges"] = dict(prims=edges, runs=[(0, len(edges))], W=W, H=Hh, base="host")
    c["edges_no_base"] = dict(c["edges"], base=None)
    # three column blocks, the last 2 columns wide; picture rows off the 16-byte grid; a list of more than two chunks of which a block keeps little;
    # the survivors order-sensitive: OVER then ADD in tile 0, ADD then OVER on the same pixels in tile 1
    W, Hh = 130, 33
    many = []
    for k in range(600):
        x, y = (k * 37) % W, (k * 11) % Hh
        many.append((x, y, 3, 2, (int(k % 256), int((3 * k) % 256), int((7 * k) % 256), 64 + k % 192), k % 3, -1, 0) if k % 5 else
                    (x, y, 5, 6, (255, int(k % 256), 0, 255 - k % 100), k % 2, (k * 3) % (FONT_W - 5), (k * 5) % (FONT_H - 6)))
    over, add = (0, 0, W, Hh, (180, 60, 20, 100), O.OVER), (0, 0, W, Hh, (90, 120, 250, 160), O.ADD)
    lo = many[:300] + [over] + many[300:] + [add]
    hi = many[:300] + [add] + many[300:] + [over]
    c["long_w130_h33"] = dict(prims=lo + hi, runs=[(0, 602), (602, 602), (0, 1204)], W=W, H=Hh, cols=2, base="host")
    # two blocks of rows (64 rows to a block), the second tile off the 16-byte grid
    c["w130_h70"] = dict(prims=_random_prims(r, 60, 130, 70), runs=[(0, 60), (10, 50)], W=130, H=70, cols=2, base="host")
    c["w64_h5"] = dict(prims=_random_prims(r, 20, 64, 5), runs=[(0, 20), (5, 10), (0, 0)], W=64, H=5, cols=3, base=None)
    # a tile as engine.spectrum_annotations lays it out, over the traces of two small spectra left on the device by a trace bank
    ann = O.spectrum_annotations(130, 33, 100030000, 2400000, 1.0, 126.0, 1024, GLYPHS, LINE_HEIGHT,
                                 markers=[dict(freq=100200000, bandwidth=200000, label="[M] 10", flags=O.CENTERLINE | O.MUTED, rgb=(200, 50, 50)),
                                          dict(freq=99500000, bandwidth=3000, sideband=O.USB, label="5", rgb=(20, 220, 90))])
    c["annotations_over_traces"] = dict(prims=ann, runs=[(0, len(ann)), (0, len(ann))], W=130, H=33, cols=2, base="trace")
    for case in c.values():
        if isinstance(case["base"], str) and case["base"] == "host":
            case["base"] = base_for(case["W"], case["H"], len(case["runs"]), case.get("cols", 1))
    return c


CASES = _cases()
TRACE_ITEMS = [dict(kind="spectrum", points=np.random.default_rng(11).uniform(0, 1, 90).astype(np.float32)),
               dict(kind="spectrum", points=np.linspace(0.1, 0.9, 200).astype(np.float32), hold=np.linspace(0.9, 0.2, 200).astype(np.float32))]
_expected = {}


def expected(name, base):
    """computed once per case and shared"""
    case = CASES[name]
    if name not in _expected:
        _expected[name] = O.atlas(case["prims"], case["runs"], case["W"], case["H"], case.get("cols", 1), base, FONT)
        _expected[name].setflags(write=False)
    return _expected[name]


def download(ctx, p, shape):
    import cubicsdr_amd.hip as H
    back = np.empty(shape, np.uint8)
    H.check(H.lib().csdr_dev_download(ctx.h, back.ctypes.data_as(C.c_void_p), C.c_void_p(p), back.nbytes))
    return back


def check_case(ctx, ov, name, tb=None):
    from cubicsdr_amd.engine import DevicePointer, overlay_prims
    case = CASES[name]
    W, Hh, cols = case["W"], case["H"], case.get("cols", 1)
    base = want_base = case["base"]
    if isinstance(base, str):                            # the picture a trace bank left on the device
        want_base = tb.render(TRACE_ITEMS, W, Hh, cols)
        assert want_base.any()
        assert tb.render(TRACE_ITEMS, W, Hh, cols, fetch=False) is None
        p, w, h = tb.device_view()
        assert (h, w) == want_base.shape[:2]
        base = DevicePointer(p, w * h)
    want = expected(name, want_base)
    keep = None if want_base is None else np.array(want_base)
    got = ov.compose(overlay_prims(case["prims"]), case["runs"], W, Hh, cols, base=base)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, len(bad), bad[:5].tolist(), got[tuple(bad[0][:2])].tolist(), want[tuple(bad[0][:2])].tolist())
    if isinstance(case["base"], str):                    # the base is never modified
        assert (download(ctx, base.ptr, want_base.shape) == want_base).all()
    elif keep is not None:
        assert (keep == case["base"]).all()
    n = len(case["runs"])
    if n % cols:                                         # the unused tiles of the last tile row
        assert not got[(n // cols) * Hh:, (n % cols) * W:].any()


def check_refusals(ctx, ov):
    """a refusal enqueues nothing and changes nothing: the last picture, the device view and the font stay"""
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import DevicePointer, overlay_prims
    case = CASES["edges"]
    args = (overlay_prims(case["prims"]), case["runs"], case["W"], case["H"], 1)
    first = ov.compose(*args, base=case["base"])
    assert (first == expected("edges", case["base"])).all()
    view = ov.device_view()
    ok, masked = (0, 0, 4, 4, (1, 2, 3, 4), 0), (0, 0, 4, 4, (1, 2, 3, 4), 0, 0, 0)
    small = np.empty(10, np.uint8)
    INV, RNG = -1, -5
    refused = [
        (dict(prims=[ok], runs=[(0, 2)]), INV), (dict(prims=[ok], runs=[(1, 1)]), INV), (dict(prims=[ok], runs=[(-1, 1)]), INV), (dict(prims=[ok], runs=[(0, -1)]), INV),
        (dict(prims=[ok], runs=[(2147483647, 2147483647)]), INV),
        (dict(prims=[ok[:5] + (3,)]), INV), (dict(prims=[ok[:5] + (-1,)]), INV),
        (dict(prims=[(0, 0, -1, 4) + ok[4:]]), INV), (dict(prims=[(0, 0, 4, -1) + ok[4:]]), INV),
        (dict(prims=[((1 << 20) + 1, 0, 4, 4) + ok[4:]]), INV), (dict(prims=[(0, -(1 << 20) - 1, 4, 4) + ok[4:]]), INV),
        (dict(prims=[masked[:6] + (FONT_W - 3, 0)]), INV), (dict(prims=[masked[:6] + (0, FONT_H - 3)]), INV), (dict(prims=[masked[:6] + (0, -1)]), INV),
        (dict(prims=[(0, 0, FONT_W + 1, 1) + masked[4:]]), INV),
        (dict(W=0), INV), (dict(W=16385), INV), (dict(H=0), INV), (dict(H=16385), INV), (dict(cols=0), INV), (dict(cols=2), INV), (dict(runs=[]), INV),
        (dict(runs=[(0, 1)] * (ov.max_tiles + 1), cols=1), RNG), (dict(prims=[ok] * (ov.max_prims + 1)), RNG), (dict(out=small), RNG),
        (dict(base=DevicePointer(view[0] + 1, 1)), INV), (dict(prims=[masked], font=None), INV),
    ]
    for call, want_rc in refused:
        if "font" in call:
            ov.set_font(None)
        rc, _ = ov.try_compose(overlay_prims(call.get("prims", [ok])), call.get("runs", [(0, 1)]), call.get("W", 8), call.get("H", 8), call.get("cols", 1),
                               base=call.get("base"), out=call.get("out"))
        if "font" in call:
            ov.set_font(FONT)
        assert rc == want_rc, (call, rc)
        assert ov.device_view() == view, call
        assert (download(ctx, view[0], first.shape) == first).all(), call
        assert (ov.compose(*args, base=case["base"]) == first).all(), call
    return len(refused)
