"""The trace bank (kernels_tracebank.hpp, csdr_tracebank.hip) through the host-thread emulation of the HIP sources (tests/emu) against the restated
rule (tests/trace_oracle.py), byte for byte, on every shared case (tests/tracebank_cases.py).  No GPU needed; the device runs the same cases in
tests/test_gpu_tracebank.py."""
import ctypes as C
import os
import sys

import pytest

from tests import tracebank_cases as K

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
def tb(ctx):
    from cubicsdr_amd.engine import TraceBank
    t = TraceBank(ctx, max_items=64, max_points=1 << 21)
    yield t
    t.close()


@pytest.mark.parametrize("name", K.EMU_CASES)
def test_emu_case(ctx, tb, name):
    K.check_case(ctx, tb, name)


def test_emu_refusals_change_nothing(tb):
    assert K.check_refusals(tb) >= 12


def test_emu_device_view_is_the_picture(ctx, tb):
    import numpy as np
    import cubicsdr_amd.hip as H
    case = K.CASES["atlas"]
    K.set_colors(tb, None)
    pic = tb.render(case["items"], case["W"], case["H"], case["cols"])
    assert tb.render(case["items"], case["W"], case["H"], case["cols"], fetch=False) is None
    p, w, h = tb.device_view()
    assert (h, w) == pic.shape[:2]
    back = np.empty_like(pic)
    H.check(H.lib().csdr_dev_download(ctx.h, back.ctypes.data_as(C.c_void_p), C.c_void_p(p), back.nbytes))
    assert (back == pic).all()
