"""The overlay bank's picture and planners (include/csdr_hip.h, "Overlay bank") restated in numpy from the header alone: the compositing rule pixel by
pixel in Python integers, the planners with numpy.longdouble / float32 where the header names those types.  Nothing here looks at the C++:
tests/test_overlay_design.py holds the planners to it, tests/test_overlay_emu.py, test_gpu_overlay.py and test_overlay_host.py the pictures.
A primitive is a tuple (x, y, w, h, (r, g, b, a), mode[, mask_x, mask_y]); modes OVER 0, ADD 1, COPY 2."""
import math

import numpy as np

OVER, ADD, COPY = 0, 1, 2
LEFT, CENTER, RIGHT = 0, 1, 2
TOP, BOTTOM = 0, 2
BOTH, USB, LSB = 0, 1, 2
DELTA_LOCK, RECORDING, MUTED, SOLO, CENTERLINE = 1, 2, 4, 8, 16
LD, F32 = np.longdouble, np.float32


def as_tuple(p):
    """a primitive from a tuple or a record of engine.PRIM_DTYPE"""
    if isinstance(p, (tuple, list)):
        return (int(p[0]), int(p[1]), int(p[2]), int(p[3]), tuple(int(v) for v in p[4]), int(p[5]), int(p[6]) if len(p) > 6 else -1, int(p[7]) if len(p) > 7 else 0)
    return (int(p["x"]), int(p["y"]), int(p["w"]), int(p["h"]), tuple(int(v) for v in p["rgba"]), int(p["mode"]), int(p["mask_x"]), int(p["mask_y"]))


def blend(d, rgba, ae, mode):
    """item 4: the four bytes d under colour rgba at effective alpha ae"""
    if mode == COPY:
        return [rgba[0], rgba[1], rgba[2], ae]
    s = (rgba[0], rgba[1], rgba[2], 255)
    if mode == OVER:
        return [(s[c] * ae + d[c] * (255 - ae) + 127) // 255 for c in range(4)]
    return [min(255, d[c] + (s[c] * ae + 127) // 255) for c in range(4)]


def paint_tile(tile, prims, font):
    """tile: [H, W, 4] uint8, modified in place: the list applied in order, vectorised over each primitive's clipped rectangle"""
    Hh, W = tile.shape[:2]
    for p in prims:
        x, y, w, h, rgba, mode, mx, my = as_tuple(p)
        x0, x1, y0, y1 = max(x, 0), min(x + w, W), max(y, 0), min(y + h, Hh)
        if x0 >= x1 or y0 >= y1:
            continue
        d = tile[y0:y1, x0:x1].astype(np.int64)
        if mx < 0:
            ae = np.full(d.shape[:2], rgba[3], np.int64)
        else:
            cov = font[my + y0 - y:my + y1 - y, mx + x0 - x:mx + x1 - x].astype(np.int64)
            ae = (rgba[3] * cov + 127) // 255
        if mode == COPY:
            out = np.stack([np.full_like(ae, rgba[0]), np.full_like(ae, rgba[1]), np.full_like(ae, rgba[2]), ae], axis=-1)
        else:
            s = np.array([rgba[0], rgba[1], rgba[2], 255], np.int64)
            a3 = ae[..., None]
            out = (s * a3 + d * (255 - a3) + 127) // 255 if mode == OVER else np.minimum(255, d + (s * a3 + 127) // 255)
        tile[y0:y1, x0:x1] = out.astype(np.uint8)


def paint_pixel(d, px, py, prims, font):
    """item 4 for ONE pixel, the slow way: what paint_tile must agree with"""
    d = [int(v) for v in d]
    for p in prims:
        x, y, w, h, rgba, mode, mx, my = as_tuple(p)
        if not (x <= px < x + w and y <= py < y + h):
            continue
        ae = rgba[3] if mx < 0 else (rgba[3] * int(font[my + py - y, mx + px - x]) + 127) // 255
        d = blend(d, rgba, ae, mode)
    return d


def atlas(prims, runs, W, Hh, cols=1, base=None, font=None):
    """items 1 - 4: -> [tile rows * H, cols * W, 4] uint8"""
    n = len(runs)
    rows = -(-n // cols)
    pic = np.zeros((rows * Hh, cols * W, 4), np.uint8)
    for k, (first, count) in enumerate(runs):
        ty, tx = divmod(k, cols)
        tile = pic[ty * Hh:(ty + 1) * Hh, tx * W:(tx + 1) * W]
        if base is not None:
            tile[:] = np.asarray(base, np.uint8).reshape(pic.shape)[ty * Hh:(ty + 1) * Hh, tx * W:(tx + 1) * W]
        paint_tile(tile, [prims[i] for i in range(first, first + count)], font)
    return pic


# ---- planners ----
def hb(u, W):
    return int(min(max(math.floor((float(u) + 1.0) * 0.5 * W), 0), W))


def vb(v, Hh):
    return int(min(max(math.floor((1.0 - float(v)) * 0.5 * Hh), 0), Hh))


def unit_byte(c):
    return int(float(c) * 255 + 0.5)


def _fixed(v, precision):
    return np.format_float_positional(v, precision=precision, unique=False, trim="k")


def freq_scale(freq, bandwidth, view_w, view_h, font_scale=1.0):
    vw, vh = F32(view_w), F32(view_h)
    left = int(float(freq) - float(bandwidth) / 2.0)
    right = int(float(left) + float(bandwidth))
    span = LD(right - left)
    step, vis, prec = (LD(100000.0) / span) * LD(2.0), 0.1, 1

    def narrow():
        return step * LD(0.5) * LD(vw) < LD(40 * font_scale)
    if narrow():
        for k, v in enumerate((0.25, 0.5, 1.0, 2.5, 5.0, 10.0, 50.0)):
            if k and not narrow():
                break
            step, vis = (LD(v * 1000000.0) / span) * LD(2.0), v
    elif step * LD(0.5) * LD(vw) > LD(350 * font_scale):
        step, vis, prec = (LD(10000.0) / span) * LD(2.0), 0.01, 2
    first = (abs(left) // 1000000) * 1000000 * (1 if left >= 0 else -1)                               # truncating division
    start = (LD(first - left) / span) * LD(2.0)
    cur = np.trunc(np.floor(LD(first) / LD(1000000.0)))
    out = dict(step_mhz=vis, precision=prec, tick_top=1.0 - (5.0 / float(vh)), label_y=1.0 - (16.0 / float(vh)) * font_scale, font_size=12)
    if vh > 135:
        out.update(font_size=16, label_y=1.0 - (18.0 / float(vh)) * font_scale)
    out.update(tick_rows=vb(out["tick_top"], view_h), label_row=vb(out["label_y"], view_h))
    ticks = []
    m, m_max = float(LD(-1.0) + start), float(LD(1.0) + abs(start))
    while m <= m_max:
        if m < -1.0:
            cur = cur + LD(vis)
        elif m > 1.0:
            break
        else:
            frac = math.modf(float(cur))[0]
            ticks.append(dict(m=m, value=float(cur), label=_fixed(cur, prec), major=frac < 0.001, column=hb(m, view_w)))
            cur = cur + LD(vis)
        m = float(LD(m) + step)
    out["ticks"] = ticks
    return out


def db_grid(floor, ceil):
    rng = float(F32(ceil) - F32(floor))
    out = []
    for r_min, r_max, trans, step in ((90.0, 5000.0, 10.0, 100.0), (20.0, 150.0, 10.0, 10.0), (-20.0, 30.0, 10.0, 1.0)):
        if not (r_min <= rng <= r_max):
            continue
        a = 1.0
        if rng <= r_min + trans:
            a *= (rng - r_min) / trans
        if rng >= r_max - trans:
            a *= (trans - (rng - (r_max - trans))) / trans
        p, ps, l = 0.0, [], float(F32(floor))
        while l <= float(F32(ceil)) + step:
            p += np.float64(step) / np.float64(rng) if rng else math.inf
            ps.append(p)
            l += step
        out.append(dict(alpha=a, step=step, p=np.array(ps, np.float64)))
    return out


def db_labels(floor, ceil, fft_size, db_offset=0.0):
    if F32(ceil) == F32(floor) or fft_size == 0:
        return "", ""

    def one(v):
        with np.errstate(all="ignore"):
            return "%.1fdB" % (db_offset + 20.0 * float(np.log10(np.float64(2.0 * float(F32(v)) / float(fft_size)))))
    return one(ceil), one(floor)


def demod_marker(demod_freq, bandwidth, sideband, center_freq, srate, flags, view_w, view_h, rgb=(255, 255, 255)):
    ux = F32(demod_freq - (center_freq - srate // 2)) / F32(srate)
    ux = F32((float(ux) - 0.5) * 2.0)
    ofs = F32(bandwidth) / F32(srate)
    ol, orr = (ofs if sideband != USB else F32(0)), (ofs if sideband != LSB else F32(0))
    lh = F32(20.0 / float(F32(view_h)))
    hp = F32(-1.0 + float(lh))
    x0, x1, ytop = hb(F32(ux - ol), view_w), hb(F32(ux + orr), view_w), vb(F32(hp + lh), view_h)
    rgb = tuple(int(v) for v in rgb)
    prims = [(x0, ytop, max(x1 - x0, 0), view_h - ytop, (0, 0, 0, 89), OVER, -1, 0), (x0, 0, max(x1 - x0, 0), view_h, rgb + (51,), ADD, -1, 0)]
    narrow = float(ofs) * 2.0 < 16.0 / float(F32(view_w))
    if narrow:
        prims.append((x0, ytop, max(x1 - x0, 0), view_h - ytop, rgb + (51,), ADD, -1, 0))
    xc = hb(ux, view_w)
    if flags & CENTERLINE and xc < view_w:
        prims.append((xc, 0, 1, view_h, rgb + (128,), ADD, -1, 0))
    letters = ("V" if flags & DELTA_LOCK else "") + ("R" if flags & RECORDING else "") + ("M" if flags & MUTED else ("S" if flags & SOLO else ""))
    return dict(ux=float(ux), ofs_left=float(ol), ofs_right=float(orr), label_v=float(hp), narrow=narrow,
                halign=LEFT if sideband == USB else (RIGHT if sideband == LSB else CENTER), label_x=xc, label_y=vb(hp, view_h),
                prefix="[%s] " % letters if letters else "", prims=prims)


def text(glyphs, line_height, s, x, y, halign=LEFT, valign=TOP, rgba=(255, 255, 255, 255), mode=OVER):
    """glyphs: records with id, x, y, w, h, xoffset, yoffset, xadvance (dicts or numpy records)"""
    def find(c):
        for g in glyphs:
            if int(g["id"]) == c:
                return g
        return None
    raw = s.encode("latin-1") if isinstance(s, str) else bytes(s)
    found = [g for g in (find(c) for c in raw) if g is not None]
    width = sum(int(g["xadvance"]) for g in found)
    pen = x if halign == LEFT else (x - width // 2 if halign == CENTER else x - width)
    top = y if valign == TOP else (y - line_height // 2 if valign == CENTER else y - line_height)
    out = []
    for g in found:
        if int(g["w"]) > 0 and int(g["h"]) > 0:
            out.append((pen + int(g["xoffset"]), top + int(g["yoffset"]), int(g["w"]), int(g["h"]), tuple(rgba), mode, int(g["x"]), int(g["y"])))
        pen += int(g["xadvance"])
    return out


def spectrum_annotations(width, height, freq, bandwidth, floor, ceil, fft_size, glyphs, line_height, markers=(), db_offset=0.0, font_scale=1.0,
                         freq_line=(255, 255, 255), text_rgb=(255, 255, 255)):
    """engine.spectrum_annotations' order: grid, ticks, MHz labels, dB labels, markers"""
    out = []
    for r in db_grid(floor, ceil):
        for p in r["p"]:
            if 0.0 <= p <= 1.0 and vb(2.0 * p - 1.0, height) < height:
                out.append((0, vb(2.0 * p - 1.0, height), width, 1, (31, 31, 31, unit_byte(r["alpha"])), ADD, -1, 0))
    sc = freq_scale(freq, bandwidth, width, height, font_scale)
    minor = tuple(int(c * 0.65 + 0.5) for c in freq_line)
    for t in sc["ticks"]:
        k = 4 if t["major"] else 1
        out.append((t["column"] - k // 2, 0, k, sc["tick_rows"], tuple(freq_line if t["major"] else minor) + (255,), OVER, -1, 0))
    for t in sc["ticks"]:
        out += text(glyphs, line_height, t["label"], t["column"], sc["label_row"], CENTER, CENTER, tuple(text_rgb) + (255,))
    hi, lo = db_labels(floor, ceil, fft_size, db_offset)
    xr = min(int(88 * font_scale), width)
    out += text(glyphs, line_height, hi, xr, 0, RIGHT, TOP, tuple(text_rgb) + (255,))
    out += text(glyphs, line_height, lo, xr, height, RIGHT, BOTTOM, tuple(text_rgb) + (255,))
    for mk in markers:
        m = demod_marker(mk["freq"], mk["bandwidth"], mk.get("sideband", BOTH), freq, bandwidth, mk.get("flags", 0), width, height, mk.get("rgb", (255, 255, 255)))
        out += m["prims"]
        out += text(glyphs, line_height, m["prefix"] + mk.get("label", ""), m["label_x"], m["label_y"], m["halign"], CENTER, (255, 255, 255, 204))
    return out
