"""The shared cases of the density bank (csdr_density; include/csdr_hip.h, "Density bank") against tests/density_oracle.py, count for count and byte
for byte: the smallest shapes at which the rule or a kernel can go wrong.  Run by the emulation (tests/test_density_emu.py), on the device
(tests/test_gpu_density.py) and, as covers, by tests/test_density_design.py.

A case is a tile size, a slot count, a list of steps (each a list of items) and a list of views; after every step the counts and peaks of ALL
slots are compared, after the last one the picture.  The kernels take another path at: 64 columns to a workgroup (W = 63, 64, 65, 300), two rows
to a plane word (odd H), 32 rows to a fold workgroup and 64 to a render workgroup (H = 129), 32 frames to a chunk (31, 32, 33 and several
chunks), a 16-byte access only where a row's cells are aligned (W = 7, 63, 65)."""
import ctypes as C
import functools

import numpy as np

from tests import density_oracle as D
from tests import tracebank_cases as TK

F32 = np.float32
CHUNK = 32                                   # kDnChunk of kernels_density.hpp
MAX_FRAMES, MAX_POINTS = 256, 8192
PALETTE = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7 + 3) % 256, (np.arange(256) * 13 + 5) % 256], axis=1).astype(np.uint8)


def _rng(seed):
    return np.random.default_rng(seed)


def frames_of(r, n, frames, kind="spectrum", layout=0, pad=0):
    """`frames` random frames of n vertices around a slowly moving level, so that covers overlap; pad: floats between frames -> (points, stride)"""
    lo, hi = (0.0, 1.0) if kind == "spectrum" else (-1.0, 1.0)
    base = r.uniform(lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo), n)
    y = (base[None, :] + r.normal(0, 0.08 * (hi - lo), (frames, n))).astype(F32)
    per = n * (1 + layout)
    buf = np.full((frames, per + pad), 123.0, F32)
    if layout:
        buf[:, 1:per:2] = y
    else:
        buf[:, :per] = y
    return buf.ravel(), per + pad


def item(r, slot, n, frames=1, kind="spectrum", layout=0, pad=0, **kw):
    p, stride = frames_of(r, n, frames, kind, layout, pad)
    return dict(slot=slot, points=p, n=n, frames=frames, kind=kind, layout=layout, stride_floats=stride, **kw)


def flat(slot, n, frames, y=0.5, **kw):
    return dict(slot=slot, points=np.full(n * frames, y, F32), n=n, frames=frames, **kw)


def decay(slot, keep):
    return dict(slot=slot, points=None, n=0, frames=0, keep_q16=keep)


def _cases():
    c = {}
    r = _rng(7)
    c["header_example"] = dict(W=7, H=10, slots=1, steps=[[dict(slot=0, points=np.array([0.95, 0.05, 0.95], F32), n=3, frames=1)]], views=[(0, 1), (0, 0)], cols=2)
    for W in (2, 7, 63, 64, 65, 300):
        for Hh in (1, 2, 10, 129):
            c["tile_%d_%d" % (W, Hh)] = dict(W=W, H=Hh, slots=2, steps=[[item(r, 0, max(2, W // 2), 3), item(r, 1, 2 * W + 1, 2, kind="y", layout=1)]],
                                            views=[(0, 0), (1, 2)])
    c["vertices_w7"] = dict(W=7, H=10, slots=6, steps=[[item(r, s, n, 2) for s, n in enumerate((1, 2, 6, 7, 8, 100))]], views=[(s, 0) for s in range(6)], cols=4)
    c["vertices_w64"] = dict(W=64, H=10, slots=3, steps=[[item(r, s, n, 2) for s, n in enumerate((63, 64, 65))]], views=[(s, 0) for s in range(3)])
    c["vertices_w300"] = dict(W=300, H=10, slots=4, steps=[[item(r, s, n, 2) for s, n in enumerate((299, 300, 301, 4097))]], views=[(3, 0)])
    counts = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 63, 64, 65, 200)
    c["frame_counts"] = dict(W=65, H=10, slots=len(counts), steps=[[item(r, s, 9, f) for s, f in enumerate(counts)]], views=[(s, 0) for s in range(len(counts))], cols=4)
    c["item_forms"] = dict(W=70, H=19, slots=4, views=[(s, 0) for s in range(4)], cols=3, palette=PALETTE,
                           steps=[[item(r, 0, 50, 5), item(r, 1, 50, 5, layout=1), item(r, 2, 90, 4, kind="y", pad=13), item(r, 3, 31, 40, kind="y", layout=1, pad=3)]])
    sp, sc = TK.boundary_values(7, 0.0, 1.0), TK.boundary_values(7, -1.0, 0.5)
    c["special_values"] = dict(W=13, H=7, slots=2, views=[(0, 0), (1, 0)],
                               steps=[[dict(slot=0, points=np.concatenate([sp, sp[::-1]]), n=sp.size, frames=2), dict(slot=1, points=sc, n=sc.size, frames=1, kind="y")]])
    c["one_slot"] = dict(W=33, H=20, slots=1, steps=[[item(r, 0, 40, 6)], [item(r, 0, 40, 3, keep_q16=40000, weight=5)]], views=[(0, 0)])
    c["slot_lists"] = dict(W=33, H=20, slots=5, views=[(s, 0) for s in range(5)], cols=2,
                           steps=[[item(r, s, 20 + s, 4, weight=1 + s) for s in range(5)],
                                  [item(r, 0, 11, 2, keep_q16=50000), item(r, 4, 70, 2), decay(3, 32768), item(r, 1, 33, 1, keep_q16=1)],      # slot 2 is absent
                                  [item(r, s, 33, 1, keep_q16=65535) for s in (4, 2)]])
    n = 16
    c["decay"] = dict(W=16, H=4, slots=4, views=[(s, 0) for s in range(4)],
                      steps=[[flat(0, n, 2), flat(1, n, 2), flat(2, n, 1), flat(3, n, 3)],
                             [flat(0, n, 1, y=0.9, keep_q16=0), flat(1, n, 1, y=0.9, keep_q16=65536), decay(2, 65535), decay(3, 32768)],
                             [decay(0, 0), decay(1, 65536), flat(2, n, 1, keep_q16=65535), flat(3, n, 3, keep_q16=32768)]])
    c["saturation"] = dict(W=4, H=3, slots=1, views=[(0, 0), (0, 1 << 31)],
                           steps=[[flat(0, 4, 255, weight=1 << 24)], [flat(0, 4, 1, weight=1 << 24)], [flat(0, 4, 1, weight=1 << 24)], [decay(0, 65536)]])
    c["render"] = dict(W=37, H=23, slots=3, palette=PALETTE, cols=4, steps=[[item(r, 0, 37, 20), item(r, 1, 80, 9, kind="y")]],
                       views=[(0, 1), (0, 0), (0, 3), (0, 1000), (-1, 0), (1, 0), (2, 0), (1, 2), (-1, 5)])      # 9 views in 4 columns: 3 unused tiles
    return c


CASES = _cases()
RANDOM_CASES = ["item_forms", "slot_lists", "render", "tile_65_129"]


@functools.lru_cache(maxsize=None)
def expected(name):
    """computed once per case and shared: the oracle's counts [steps][slots, H, W], and its picture"""
    case = CASES[name]
    bank = D.Bank(case["W"], case["H"], case["slots"])
    states = []
    for items in case["steps"]:
        bank.step(items)
        states.append(bank.count.copy())
    pic = D.render(bank, case["views"], case.get("cols", 1), case.get("palette"))
    for a in states:
        a.setflags(write=False)
    pic.setflags(write=False)
    return states, pic


def check_preconditions():
    """asserted on the oracle's own output, so that no case passes vacuously"""
    states, _ = expected("header_example")
    lo, hi = [0, 2, 7, 2, 0], [2, 7, 9, 7, 2]
    want = np.zeros((10, 7), np.uint32)
    for col in range(5):
        want[lo[col]:hi[col] + 1, col] = 1
    assert (states[0][0] == want).all()
    for name in RANDOM_CASES:
        first = expected(name)[0][0]
        case = CASES[name]
        cov = [D.item_cover(it, case["W"], case["H"]) for it in case["steps"][0]]
        assert any((v == 0).any() and (v == 1).any() and (v >= 2).any() for v in cov), name
        assert first.max() >= 2, name
    it = CASES["item_forms"]["steps"][0][0]
    lo, hi = D.frame_interval(it["points"][:it["n"]], it["n"], 0, "spectrum", 70, 19)
    assert (hi - lo >= 1).any() and (hi < 0).any()                   # a column's interval longer than one row; an unlit column (n = 50 < W = 70)
    render_peak = int(expected("render")[0][-1][0].max())            # the render case draws slot 0 with `full` 3 and 1000: below and above its peak
    assert 3 < render_peak < 1000, render_peak
    states, _ = expected("decay")
    assert states[0][2].max() == 1 and states[1][2].max() == 0       # keep 65535 takes 1 to 0
    assert states[0][3].max() == 3 and states[1][3].max() == 1       # keep 32768 takes 3 to 1: the floor drops a half
    assert states[1][0].max() == 1 and (states[1][0][states[0][0] == 2] == 0).all()      # keep 0 forgets
    assert (states[1][1] >= states[0][1]).all() and states[1][1].max() == 2 and (states[2][1] == states[1][1]).all()
    states, _ = expected("saturation")
    assert states[0].max() == 255 << 24 and states[1].max() == D.SAT and states[2].max() == D.SAT and states[3].max() == D.SAT
    return True


def upload(ctx, it, allocs):
    """the same item with its points in device memory"""
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import DevicePointer
    if it.get("points") is None:
        return it
    a = np.ascontiguousarray(it["points"], F32).ravel()
    p = C.c_void_p()
    H.check(H.lib().csdr_dev_alloc(ctx.h, max(a.nbytes, 4), C.byref(p)))
    allocs.append(p)
    H.check(H.lib().csdr_dev_upload(ctx.h, p, a.ctypes.data_as(C.c_void_p), a.nbytes))
    return dict(it, points=DevicePointer(p.value, a.size))


def free(ctx, allocs):
    import cubicsdr_amd.hip as H
    for p in allocs:
        H.check(H.lib().csdr_dev_free(ctx.h, p))


def mismatch(got, want):
    bad = np.argwhere(got != want)
    return None if bad.size == 0 else (len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def check_case(ctx, db, name, dev=False):
    case = CASES[name]
    states, pic = expected(name)
    db.setup(case["W"], case["H"], case["slots"], MAX_FRAMES, MAX_POINTS)
    db.set_palette(D.DEFAULT_PALETTE if case.get("palette") is None else case["palette"])
    allocs = []
    try:
        for k, items in enumerate(case["steps"]):
            db.step([upload(ctx, it, allocs) if dev else it for it in items])
            for s in range(case["slots"]):
                got = db.fetch(s)                                    # (synchronises: the device points may go)
                assert mismatch(got, states[k][s]) is None, (name, "step", k, "slot", s, mismatch(got, states[k][s]))
                assert db.peak(s) == int(states[k][s].max()), (name, "peak", k, s)
    finally:
        free(ctx, allocs)
    got = db.render(case["views"], case.get("cols", 1))
    assert got.shape == pic.shape
    assert mismatch(got, pic) is None, (name, "picture", mismatch(got, pic))
    db.reset_slot(0)
    assert not db.fetch(0).any() and db.peak(0) == 0


def check_refusals(db):
    """a refusal changes nothing: against an undisturbed twin (the oracle's state of the same steps)"""
    r = _rng(11)
    W, Hh = 20, 9
    db.setup(W, Hh, 3, 8, 64)
    db.set_palette(D.DEFAULT_PALETTE)
    twin = D.Bank(W, Hh, 3)
    first = [item(r, 0, 30, 4), item(r, 1, 10, 2, kind="y"), item(r, 2, 20, 1)]
    db.step(first)
    twin.step(first)
    ok = dict(slot=1, points=np.linspace(0, 1, 16).astype(F32), n=16, frames=1)
    refused = [
        ([ok, dict(ok, slot=0), dict(ok)], -1),                      # a slot named twice
        ([dict(ok, kind=2)], -1), ([dict(ok, kind=3)], -1), ([dict(ok, kind=-1)], -1),
        ([dict(ok, layout=2)], -1), ([dict(ok, layout=-1)], -1),
        ([dict(ok, points=np.zeros(32, F32), frames=2, stride_floats=15)], -1),              # stride too small
        ([dict(ok, points=np.zeros(64, F32), frames=2, layout=1, stride_floats=31)], -1),
        ([dict(ok, slot=0), dict(ok, points=np.zeros(65, F32), n=65)], -5),                    # n above max_points
        ([dict(ok, slot=0), dict(ok, points=np.zeros(9 * 16, F32), frames=9)], -5),            # frames above max_frames
        ([dict(ok, weight=0)], -1), ([dict(ok, weight=(1 << 24) + 1)], -1), ([dict(ok, keep_q16=65537)], -1),
        ([dict(ok, slot=3)], -1), ([dict(ok, slot=-1)], -1), ([dict(ok, n=-1)], -1), ([dict(ok, frames=-1)], -1), ([], -1),
        ([dict(ok, slot=s % 3) for s in range(4)], -1),             # more items than slots
    ]
    for items, want in refused:
        rc = db.try_step(items)
        assert rc == want, (items and {k: v for k, v in items[-1].items() if k != "points"}, rc)
        for s in range(3):
            assert (db.fetch(s) == twin.count[s]).all(), (rc, s)
    pic = db.render([(0, 0), (1, 0), (2, 0)], 2)
    for views, cols, want in (([(3, 0)], 1, -1), ([(-2, 0)], 1, -1), ([(0, 0)], 2, -1), ([(0, 0)], 0, -1), ([], 1, -1)):
        rc, _ = db.try_render(views, cols)
        assert rc == want, (views, cols, rc)
    rc, _ = db.try_render([(0, 0)], 1, out=np.empty(10, np.uint8))
    assert rc == -5
    assert (db.render([(0, 0), (1, 0), (2, 0)], 2) == pic).all() and (pic == D.render(twin, [(0, 0), (1, 0), (2, 0)], 2)).all()
    for s in range(3):
        assert (db.fetch(s) == twin.count[s]).all()
    return len(refused)
