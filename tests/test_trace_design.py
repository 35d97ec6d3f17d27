"""csdr_design_trace_envelope (host only: the real library, no device) against the restatement of the rule in tests/trace_oracle.py, on the shared
cases and on 2000 seeded random (n, W, H); on the random ones also the three properties the header states: every column up to c_{n-1} is lit, every
vertex's row lies in its column's interval, the intervals of adjacent columns share a row."""
import ctypes as C

import numpy as np
import pytest

from tests import trace_oracle as O
from tests import tracebank_cases as K


@pytest.fixture(scope="module")
def design():
    from cubicsdr_amd import build
    build.build(verbose=False)
    from cubicsdr_amd.engine import design_trace_envelope
    return design_trace_envelope


def both(design, it, W, H):
    kind = O.KINDS[it["kind"]]
    layout = it.get("layout", 0)
    n = np.asarray(it["points"]).size // (1 + layout)
    got = design(it["points"], W, H, kind, hold=it.get("hold"), layout=layout, n=n)
    want = O.design_envelope(it["points"], n, layout, kind, W, H, hold=it.get("hold"))
    return got, want


@pytest.mark.parametrize("name", list(K.CASES))
def test_envelope_of_the_cases(design, name):
    case = K.CASES[name]
    seen = 0
    for it in case["items"]:
        if it is None or it["points"] is None or it["kind"] == "xy":
            continue
        (lo, hi), (wlo, whi) = both(design, it, case["W"], case["H"])
        assert (lo == wlo).all() and (hi == whi).all(), name
        seen += 1
    assert seen or name.startswith("xy")


def test_the_example_of_the_header(design):
    lo, hi = design(np.array([0.95, 0.05, 0.95], np.float32), 7, 10)
    assert lo[0].tolist() == [0, 2, 7, 2, 0, -1, -1] and hi[0].tolist() == [2, 7, 9, 7, 2, -1, -1]
    assert (lo[1] == -1).all() and (hi[1] == -1).all()


def test_random_envelopes_and_their_properties(design):
    rng = np.random.default_rng(7)
    for k in range(2000):
        n = int(rng.integers(1, 400)) if k % 4 else int(rng.integers(1, 6))
        W = int(rng.integers(2, 200))
        H = int(rng.integers(1, 70))
        kind = ("spectrum", "y")[k % 2]
        y = rng.uniform(-0.2, 1.2, n).astype(np.float32) if kind == "spectrum" else rng.uniform(-1.2, 1.2, n).astype(np.float32)
        it = dict(kind=kind, points=K.pairs(y) if k % 3 == 0 else y, layout=1 if k % 3 == 0 else 0)
        (lo, hi), (wlo, whi) = both(design, it, W, H)
        assert (lo == wlo).all() and (hi == whi).all(), (n, W, H, kind)
        lo, hi = lo[0].astype(np.int64), hi[0].astype(np.int64)
        cols = np.arange(n, dtype=np.int64) * W // n
        last = cols[-1]
        assert (lo[:last + 1] >= 0).all() and (lo[last + 1:] == -1).all() and (hi[last + 1:] == -1).all(), (n, W, H)
        rows = O.polylines(O.KINDS[kind], it["points"], None, n, it["layout"], H)[0]
        assert ((lo[cols] <= rows) & (rows <= hi[cols])).all(), (n, W, H)
        assert (np.maximum(lo[:last], lo[1:last + 1]) <= np.minimum(hi[:last], hi[1:last + 1])).all(), (n, W, H)


def test_two_y_writes_both_sub_panels(design):
    y = np.linspace(-1, 1, 20).astype(np.float32)
    lo, hi = design(y, 10, 9, "2y")
    assert (lo[0] >= 0).all() and (hi[0] <= 3).all() and (lo[1] >= 4).all() and (hi[1] <= 8).all()


def test_refusals():
    from cubicsdr_amd import build, hip
    build.build(verbose=False)
    lib = hip.lib()
    y = np.linspace(0, 1, 8).astype(np.float32)
    lo, hi = (np.zeros(2 * 16, np.int32) for _ in range(2))
    p, L, Hh = y.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)
    assert lib.csdr_design_trace_envelope(p, None, 8, 0, 0, 16, 4, L, Hh) == 0
    for args in ((p, None, 8, 0, 4, 16, 4, L, Hh), (p, None, 8, 0, 3, 16, 4, L, Hh), (p, None, 8, 2, 0, 16, 4, L, Hh), (p, None, -1, 0, 0, 16, 4, L, Hh),
                 (p, None, 8, 0, 0, 1, 4, L, Hh), (p, None, 8, 0, 0, 16, 0, L, Hh), (p, None, 8, 0, 2, 16, 1, L, Hh), (None, None, 8, 0, 0, 16, 4, L, Hh),
                 (p, None, 8, 0, 0, 16, 4, None, Hh)):
        assert lib.csdr_design_trace_envelope(*args) == -1, args[2:7]
    assert lib.csdr_design_trace_envelope(p, None, (1 << 21) + 1, 0, 0, 16, 4, L, Hh) == -5
    assert lib.csdr_design_trace_envelope(None, None, 0, 0, 0, 16, 4, L, Hh) == 0 and (lo == -1).all() and (hi == -1).all()
