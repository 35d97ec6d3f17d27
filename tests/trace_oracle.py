"""The drawing rule of the trace bank restated from the header text alone (include/csdr_hip.h, "Trace bank", items 1 - 6): plain integers, and
numpy.float32 for the one float step per vertex.  Nothing here looks at the C++: tests/test_trace_design.py holds csdr_design_trace_envelope to it,
the emulation and GPU tests hold the pictures to it byte for byte."""
import numpy as np

F32 = np.float32
SPECTRUM, SCOPE_Y, SCOPE_2Y, SCOPE_XY = range(4)
KINDS = {"spectrum": SPECTRUM, "y": SCOPE_Y, "2y": SCOPE_2Y, "xy": SCOPE_XY}
DEFAULT_COLORS = dict(bg=(0, 0, 0, 255), line=(255, 255, 255), hold=(0, 255, 0), axis_major=(255, 255, 255), axis_minor=(89, 89, 89))


def quant(y, y0, s, N):
    """item 1: q of every value of y (float32) for the constants (y0, s) in a panel of N rows (or columns) -> int64 array"""
    y = np.atleast_1d(np.asarray(y, F32))
    with np.errstate(all="ignore"):
        u = (y - F32(y0)) * F32(s)                      # float32 arrays: every operation is rounded to float32 on its own
        q = np.floor(u * F32(N))
    out = np.zeros(y.shape, np.int64)                   # u < 0, -0.0 and NaN
    inside = (u > 0) & (u < 1)
    out[inside] = np.clip(q[inside].astype(np.int64), 0, N - 1)
    out[u >= 1] = N - 1                                 # u >= 1 and +inf
    return out


def rdiv(p, q):
    return (2 * p + q) // (2 * q)                       # (// floors, for negative p too)


def envelope(rows, W):
    """items 2 and 3: the lit interval of every column for a polyline whose vertices lie in `rows` -> (lo, hi), -1 where unlit"""
    rows = np.asarray(rows, np.int64)
    n = rows.size
    big = 1 << 40
    lo, hi = np.full(W, big, np.int64), np.full(W, -1, np.int64)
    if n:
        c = np.arange(n, dtype=np.int64) * W // n
        np.minimum.at(lo, c, rows)                      # a == b gives {ra, rb} to the column; t = 0 and t = 2 d give ra to column a and rb to column b
        np.maximum.at(hi, c, rows)
        a, b, ra, rb = c[:-1], c[1:], rows[:-1], rows[1:]
        for k in np.nonzero(b > a)[0]:
            d = int(b[k] - a[k])
            cols = np.arange(a[k], b[k] + 1)
            for sign in (-1, 1):
                t = np.clip(2 * (cols - a[k]) + sign, 0, 2 * d)
                r = ra[k] + rdiv((rb[k] - ra[k]) * t, 2 * d)
                lo[cols] = np.minimum(lo[cols], r)
                hi[cols] = np.maximum(hi[cols], r)
    lo[hi < 0] = -1
    return lo, hi


def values(points, n, layout):
    """the y of the n vertices of a line kind"""
    p = np.asarray(points, F32).ravel()
    return p[1:2 * n:2] if layout else p[:n]


def polylines(kind, points, hold, n, layout, H):
    """item 4 -> [(rows of the vertices in TILE rows) for the line / upper sub-panel, the same for the hold / lower sub-panel or None]"""
    if kind == SPECTRUM:
        ys = values(points, n, layout)
        first = H - 1 - quant(ys, 0, 1, H)
        return [first, None if hold is None else H - 1 - quant(values(hold, n, layout), 0, 1, H)]
    if kind == SCOPE_Y:
        return [H - 1 - quant(values(points, n, layout), -1, 0.5, H), None]
    ys = values(points, n, layout)
    m, hu = n // 2, H // 2
    hl = H - hu
    return [hu - 1 - quant(ys[:m], -1, 0.5, hu), hu + hl - 1 - quant(ys[m:2 * m], -1, 0.5, hl)]


def design_envelope(points, n, layout, kind, W, H, hold=None):
    """what csdr_design_trace_envelope writes: (lo, hi), int64 [2, W]"""
    lo, hi = np.full((2, W), -1, np.int64), np.full((2, W), -1, np.int64)
    if n > 0:
        for w, rows in enumerate(polylines(kind, points, hold, n, layout, H)):
            if rows is not None:
                lo[w], hi[w] = envelope(rows, W)
    return lo, hi


def tile(item, W, H, colors=None):
    """one tile, [H, W, 4] uint8; item: None or a dict(kind, points, hold, n, layout)"""
    col = dict(DEFAULT_COLORS, **(colors or {}))
    pic = np.zeros((H, W, 4), np.uint8)
    if item is None or item.get("points") is None:
        return pic
    kind = KINDS[item["kind"]] if isinstance(item["kind"], str) else item["kind"]
    layout = item.get("layout", 0)
    floats = np.asarray(item["points"], F32).ravel()
    n = item.get("n")
    if n is None:
        n = floats.size if kind == SCOPE_XY else floats.size // (1 + layout)
    if n == 0:
        return pic
    pic[:] = col["bg"]
    rgb = pic[:, :, :3]
    if kind == SCOPE_XY:
        pts = floats[:n // 2 * 2].reshape(-1, 2)
        hits = np.zeros((H, W), np.int64)
        np.add.at(hits, (H - 1 - quant(pts[:, 1], -1, 0.5, H), quant(pts[:, 0], -1, 0.5, W)), 1)
        rgb[:] = np.minimum(255, np.asarray(col["bg"][:3], np.int64) + hits[:, :, None] * np.asarray(col["line"], np.int64))
        return pic
    if kind == SCOPE_Y:
        rgb[H - 1 - quant(0.0, -1, 0.5, H)[0]] = col["axis_minor"]
    if kind == SCOPE_2Y:
        hu = H // 2
        hl = H - hu
        rgb[hu - 1 - quant(0.0, -1, 0.5, hu)[0]] = col["axis_minor"]
        rgb[hu + hl - 1 - quant(0.0, -1, 0.5, hl)[0]] = col["axis_minor"]
        rgb[hu] = col["axis_major"]
    first, second = polylines(kind, floats, item.get("hold"), n, layout, H)
    r = np.arange(H)[:, None]
    lo, hi = envelope(first, W)
    rgb[(r >= lo) & (r <= hi)] = col["line"]
    if second is not None:
        lo, hi = envelope(second, W)
        m = (r >= lo) & (r <= hi)
        if kind == SPECTRUM:
            rgb[m] = ((rgb[m].astype(np.int64) + np.asarray(col["hold"], np.int64) + 1) >> 1).astype(np.uint8)
        else:
            rgb[m] = col["line"]
    return pic


def atlas(items, W, H, atlas_cols=1, colors=None):
    """item 6 -> [ceil(len(items) / atlas_cols) * H, atlas_cols * W, 4] uint8"""
    rows = -(-len(items) // atlas_cols)
    pic = np.zeros((rows * H, atlas_cols * W, 4), np.uint8)
    for k, it in enumerate(items):
        ty, tx = divmod(k, atlas_cols)
        pic[ty * H:(ty + 1) * H, tx * W:(tx + 1) * W] = tile(it, W, H, colors)
    return pic
