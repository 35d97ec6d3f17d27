"""The density bank (kernels_density.hpp, csdr_density.hip) through the host-thread emulation of the HIP sources (tests/emu) against the restated
rule (tests/density_oracle.py): counts, peaks and pictures byte for byte on every shared case (tests/density_cases.py), and the refusals.  No GPU
needed; the device runs the same cases in tests/test_gpu_density.py."""
import ctypes as C
import os
import sys

import pytest

from tests import density_cases as K

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
def db(ctx):
    from cubicsdr_amd.engine import DensityBank
    d = DensityBank(ctx, 8, 8, 1, K.MAX_FRAMES, K.MAX_POINTS)
    yield d
    d.close()


@pytest.mark.parametrize("name", list(K.CASES))
def test_emu_case(ctx, db, name):
    K.check_case(ctx, db, name)


def test_emu_refusals_change_nothing(db):
    assert K.check_refusals(db) >= 12


def test_emu_device_view_is_the_picture(ctx, db):
    import numpy as np
    import cubicsdr_amd.hip as H
    case = K.CASES["render"]
    K.check_case(ctx, db, "render")                      # (leaves slot 0 reset)
    pic = db.render(case["views"], case["cols"])
    assert db.render(case["views"], case["cols"], fetch=False) is None
    p, w, h = db.device_view()
    assert (h, w) == pic.shape[:2]
    back = np.empty_like(pic)
    H.check(H.lib().csdr_dev_download(ctx.h, back.ctypes.data_as(C.c_void_p), C.c_void_p(p), back.nbytes))
    assert (back == pic).all() and pic[:, :, 3].any()
