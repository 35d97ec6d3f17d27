"""The shared cases of the trace bank (csdr_tracebank; include/csdr_hip.h, "Trace bank") against tests/trace_oracle.py, byte for byte: the smallest
shapes at which the rule or a kernel can go wrong.  Run by the emulation (tests/test_tracebank_emu.py), on the device (tests/test_gpu_tracebank.py)
and, as envelopes, by tests/test_trace_design.py."""
import ctypes as C

import numpy as np

from tests import trace_oracle as O

F32 = np.float32
OTHER_COLORS = dict(bg=(10, 20, 30, 200), line=(250, 128, 3), hold=(1, 255, 77), axis_major=(200, 100, 50), axis_minor=(9, 8, 7))


def pairs(y, x=7.0):
    """layout 1: (x, y) pairs whose x the line kinds never read"""
    y = np.asarray(y, F32)
    return np.stack([np.full(y.shape, x, F32), y], axis=1).ravel()


def boundary_values(H, y0, s):
    """values just either side of every row boundary of a panel of H rows, and the special ones"""
    k = np.arange(H + 1, dtype=np.float64) / H / s + y0
    v = np.asarray(k, F32)
    out = np.concatenate([np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))])
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.99999994, 1.0, -1.0, np.nextafter(F32(-1), F32(0)), 1e-45, -1e-45, 3e38, -3e38], F32)
    return np.concatenate([special, out, special[::-1]]).astype(F32)


def _rng(seed):
    return np.random.default_rng(seed)


def _cases():
    c = {}
    r = _rng(1)

    def spec(y, hold=None, layout=0):
        it = dict(kind="spectrum", points=pairs(y) if layout else np.asarray(y, F32), layout=layout)
        if hold is not None:
            it["hold"] = pairs(hold, -3.0) if layout else np.asarray(hold, F32)
        return it

    def scope(kind, y, layout=0):
        return dict(kind=kind, points=pairs(y) if layout else np.asarray(y, F32), layout=layout)
    c["w2_h1"] = dict(items=[spec([0.2, 0.9, 0.5])], W=2, H=1)
    c["n1"] = dict(items=[spec([0.55]), scope("y", [0.3]), scope("2y", [0.3]), scope("2y", [0.3, -0.4], 1)], W=7, H=10, cols=2)
    c["rows_0_9_0"] = dict(items=[spec([0.95, 0.05, 0.95])], W=7, H=10)
    c["n_eq_w"] = dict(items=[spec(r.uniform(-0.1, 1.1, 37))], W=37, H=23)
    c["n_2w_plus_1"] = dict(items=[spec(r.uniform(-0.1, 1.1, 75), layout=1)], W=37, H=23)
    c["n4096_w100"] = dict(items=[spec(r.uniform(0, 1, 4096)), scope("y", r.uniform(-1, 1, 4096), 1)], W=100, H=33)
    c["alternating"] = dict(items=[spec(np.arange(300) % 2), scope("y", (np.arange(301) % 2) * 2.0 - 1.0)], W=70, H=19)
    c["sparse"] = dict(items=[spec(r.uniform(0, 1, 5)), scope("y", r.uniform(-1, 1, 2), 1)], W=200, H=50)
    c["special_values"] = dict(items=[spec(boundary_values(7, 0.0, 1.0)), scope("y", boundary_values(7, -1.0, 0.5)), scope("2y", boundary_values(7, -1.0, 0.5), 1)],
                               W=13, H=14)
    c["rows_in_groups"] = dict(items=[spec(r.uniform(0, 1, 700), hold=r.uniform(0, 1, 700))], W=130, H=100)
    c["past_2_31"] = dict(items=[spec(_rng(2).uniform(-0.2, 1.2, 1 << 21).astype(F32))], W=16384, H=8)
    c["two_y"] = dict(items=[scope("2y", r.uniform(-1.2, 1.2, 14)), scope("2y", r.uniform(-1, 1, 15), 1), scope("2y", r.uniform(-1, 1, 301))], W=21, H=9, cols=3)
    c["two_y_h2"] = dict(items=[scope("2y", r.uniform(-1, 1, 40))], W=16, H=2)
    xy = r.uniform(-1.1, 1.1, (500, 2)).astype(F32)
    xy[:100] = (0.25, -0.5)                              # one pixel hit 100 times
    xy[100:104] = [(-1, -1), (1, 1), (-1, 1), (1, -1)]
    xy[104] = (np.nan, 0.0)
    xy[105] = (0.0, np.nan)
    xy[110:160] = (-0.5, 0.5)                            # and one 50 times: only the blue channel saturates
    c["xy"] = dict(items=[dict(kind="xy", points=xy.ravel())], W=20, H=12, colors=dict(bg=(10, 0, 250, 255), line=(3, 3, 3)))
    c["xy_rows_in_groups"] = dict(items=[dict(kind="xy", points=r.uniform(-1, 1, 2001).astype(F32)), dict(kind="xy", points=np.zeros(1, F32))], W=9, H=300)
    up, down = np.linspace(0.05, 0.9, 128), np.linspace(0.95, 0.1, 128)
    c["hold_crossing"] = dict(items=[spec(up, hold=down), spec(down, hold=up, layout=1)], W=50, H=40)
    a = spec(r.uniform(0, 1, 90), hold=r.uniform(0, 1, 90))
    mixed = [a, None, scope("y", r.uniform(-1, 1, 64), 1), a, dict(kind="xy", points=r.uniform(-1, 1, 400).astype(F32))]
    c["atlas"] = dict(items=mixed, W=30, H=21, cols=2)
    c["atlas_colors"] = dict(items=mixed[::-1] + [scope("2y", r.uniform(-1, 1, 128), 1), dict(kind="y", points=None)], W=33, H=20, cols=3, colors=OTHER_COLORS)
    return c


CASES = _cases()
EMU_CASES = list(CASES)


def expected(case):
    return O.atlas(case["items"], case["W"], case["H"], case.get("cols", 1), case.get("colors"))


def set_colors(tb, colors):
    tb.set_colors(**dict(O.DEFAULT_COLORS, **(colors or {})))


def upload(ctx, item, allocs):
    """the same item with its points (and hold) in device memory"""
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import DevicePointer
    it = dict(item)
    for key in ("points", "hold"):
        a = item.get(key)
        if a is None:
            continue
        a = np.ascontiguousarray(a, F32).ravel()
        p = C.c_void_p()
        H.check(H.lib().csdr_dev_alloc(ctx.h, max(a.nbytes, 4), C.byref(p)))
        allocs.append(p)
        if a.nbytes:
            H.check(H.lib().csdr_dev_upload(ctx.h, p, a.ctypes.data_as(C.c_void_p), a.nbytes))
        it[key] = DevicePointer(p.value, a.size)
    return it


def free(ctx, allocs):
    import cubicsdr_amd.hip as H
    for p in allocs:
        H.check(H.lib().csdr_dev_free(ctx.h, p))


def check_case(ctx, tb, name, dev=False):
    case = CASES[name]
    set_colors(tb, case.get("colors"))
    want = expected(case)
    allocs = []
    try:
        items = [it if it is None or not dev else upload(ctx, it, allocs) for it in case["items"]]
        got = tb.render(items, case["W"], case["H"], case.get("cols", 1))
    finally:
        free(ctx, allocs)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, len(bad), bad[:5].tolist(), got[tuple(bad[0][:2])].tolist(), want[tuple(bad[0][:2])].tolist())


def check_refusals(tb):
    """a refusal renders nothing and changes nothing: the previous valid call, repeated, gives the same bytes"""
    case = CASES["atlas"]
    set_colors(tb, None)
    args = (case["items"], case["W"], case["H"], case["cols"])
    first = tb.render(*args)
    assert (first == expected(case)).all()
    y = np.linspace(0, 1, 16).astype(F32)
    ok = dict(kind="spectrum", points=y)
    small = np.empty(10, np.uint8)
    refused = [
        (([dict(ok, kind=4)], 8, 8), None), (([dict(ok, kind=-1)], 8, 8), None), (([dict(ok, layout=2, n=8)], 8, 8), None),
        (([dict(ok, n=-1)], 8, 8), None), (([ok], 1, 8), None), (([ok], 16385, 8), None), (([ok], 8, 0), None), (([ok], 8, 16385), None),
        (([ok], 8, 8, 0), None), (([ok], 8, 8, 2), None), (([], 8, 8), None), (([dict(kind="2y", points=y)], 8, 1), None),
        (([ok, dict(ok, points=np.zeros(tb.max_points + 1, F32))], 8, 8), "range"), (([ok] * (tb.max_items + 1), 8, 8), None),
        (([ok], 8, 8, 1, small), "range"),
    ]
    for call, what in refused:
        rc, _ = tb.try_render(*call)
        assert rc == (-5 if what == "range" else -1), (call[1:], rc)
        again = tb.render(*args)
        assert (again == first).all(), call[1:]
    return len(refused)
