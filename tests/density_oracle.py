"""The rule of the density bank restated from the header text alone (include/csdr_hip.h, "Density bank", items 1 - 4): numpy and Python integers.
The cover of a frame is the trace bank's line interval, taken unchanged from tests/trace_oracle.py (polylines, envelope).  Nothing here looks at
the C++: tests/test_density_design.py holds csdr_design_density_cover to it, the emulation and GPU tests hold counts, peaks and pictures to it."""
import numpy as np

from tests import trace_oracle as O

F32 = np.float32
KINDS = {"spectrum": O.SPECTRUM, "y": O.SCOPE_Y}
SAT = (1 << 32) - 1


def frame_interval(points, n, layout, kind, W, H):
    """item 1: (lo, hi) of every column for one frame, -1 where unlit"""
    rows = O.polylines(KINDS[kind] if isinstance(kind, str) else kind, points, None, n, layout, H)[0]
    return O.envelope(rows, W)


def cover(points, n, layout, stride_floats, frames, kind, W, H):
    """item 1: cover[r][c] = frames f with lo_c(f) <= r <= hi_c(f) -> int64 [H, W]"""
    out = np.zeros((H, W), np.int64)
    if points is None or n == 0 or frames == 0:
        return out
    p = np.asarray(points, F32).ravel()
    r = np.arange(H)[:, None]
    for f in range(frames):
        lo, hi = frame_interval(p[f * stride_floats:f * stride_floats + n * (1 + layout)], n, layout, kind, W, H)
        out += (hi >= 0) & (r >= lo) & (r <= hi)
    return out


def item_cover(item, W, H):
    layout, frames = item.get("layout", 0), item.get("frames", 1)
    p = item.get("points")
    if p is None:
        return np.zeros((H, W), np.int64)
    n = item.get("n")
    if n is None:
        n = np.asarray(p).size // max(frames, 1) // (1 + layout)
    stride = item.get("stride_floats", n * (1 + layout))
    return cover(p, n, layout, stride, frames, item.get("kind", "spectrum"), W, H)


def step_cells(count, keep_q16, weight, cov):
    """item 2, cell by cell in Python integers -> uint32 array"""
    flat = [min(SAT, (int(c) * int(keep_q16)) // 65536 + int(weight) * int(v)) for c, v in zip(count.ravel().tolist(), cov.ravel().tolist())]
    return np.array(flat, np.uint64).astype(np.uint32).reshape(count.shape)


class Bank:
    """items 2 and 3: the state of every slot"""

    def __init__(self, W, H, max_slots):
        self.W, self.H = W, H
        self.count = np.zeros((max_slots, H, W), np.uint32)

    def step(self, items):
        for it in items:
            s = it["slot"]
            self.count[s] = step_cells(self.count[s], it.get("keep_q16", 65536), it.get("weight", 1), item_cover(it, self.W, self.H))

    def reset_slot(self, s):
        self.count[s] = 0

    def peak(self, s):
        return int(self.count[s].max())


def index(count, full_eff):
    """item 4: the palette index of every count, Python integers"""
    out = []
    for c in count.ravel().tolist():
        out.append(0 if c == 0 else (255 if c >= full_eff else max(1, (c * 255) // full_eff)))
    return np.array(out, np.int64).reshape(count.shape)


DEFAULT_PALETTE = np.stack([np.arange(256)] * 3 + [np.full(256, 255)], axis=1).astype(np.uint8)


def render(bank, views, atlas_cols=1, palette=None):
    """item 4 -> [ceil(len(views) / atlas_cols) * H, atlas_cols * W, 4] uint8"""
    pal = DEFAULT_PALETTE if palette is None else np.asarray(palette, np.uint8).reshape(256, 4)
    W, H = bank.W, bank.H
    rows = -(-len(views) // atlas_cols)
    pic = np.zeros((rows * H, atlas_cols * W, 4), np.uint8)
    for k, (slot, full) in enumerate(views):
        if slot < 0:
            continue
        full_eff = full if full else max(bank.peak(slot), 1)
        ty, tx = divmod(k, atlas_cols)
        pic[ty * H:(ty + 1) * H, tx * W:(tx + 1) * W] = pal[index(bank.count[slot], full_eff)]
    return pic
