"""The overlay bank (kernels_overlay.hpp, csdr_overlay.hip) through the host-thread emulation of the HIP sources (tests/emu) against the restated
rule (tests/overlay_oracle.py), byte for byte, on every shared case (tests/overlay_cases.py).  No GPU needed; the device runs the same cases in
tests/test_gpu_overlay.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import overlay_cases as K
from tests import overlay_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))


@pytest.fixture(scope="module")
def ctx():
    import build_emu
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import Context
    path = build_emu.build(os.environ.get("CSDR_EMU_FLAVOR", ""))
    lib = C.CDLL(path)
    for name, (res, args) in H.ABI.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    saved = H._lib
    H._lib = lib
    c = Context(0)
    try:
        yield c
    finally:
        c.close()
        H._lib = saved


@pytest.fixture(scope="module")
def ov(ctx):
    from cubicsdr_amd.engine import OverlayBank
    o = OverlayBank(ctx, max_tiles=16, max_prims=2048)
    o.set_font(K.FONT)
    yield o
    o.close()


@pytest.fixture(scope="module")
def tb(ctx):
    from cubicsdr_amd.engine import TraceBank
    t = TraceBank(ctx, max_items=4, max_points=4096)
    yield t
    t.close()


def test_the_oracle_agrees_with_itself_pixel_by_pixel():
    """the vectorised oracle against the rule applied to single pixels, on the case with every edge"""
    case = K.CASES["edges"]
    want = K.expected("edges", case["base"])
    r = np.random.default_rng(0)
    for _ in range(200):
        py, px = int(r.integers(0, case["H"])), int(r.integers(0, case["W"]))
        assert O.paint_pixel(case["base"][py, px], px, py, case["prims"], K.FONT) == want[py, px].tolist()


@pytest.mark.parametrize("name", list(K.CASES))
def test_emu_case(ctx, ov, tb, name):
    K.check_case(ctx, ov, name, tb)


def test_emu_refusals_change_nothing(ctx, ov):
    assert K.check_refusals(ctx, ov) >= 20


def test_emu_device_view_is_the_picture(ctx, ov):
    from cubicsdr_amd.engine import overlay_prims
    case = K.CASES["atlas_w7_h5"]
    args = (overlay_prims(case["prims"]), case["runs"], case["W"], case["H"], case["cols"])
    pic = ov.compose(*args, base=case["base"])
    assert ov.compose(*args, base=case["base"], fetch=False) is None
    p, w, h = ov.device_view()
    assert (h, w) == pic.shape[:2]
    assert (K.download(ctx, p, pic.shape) == pic).all()
