"""The view bank (viewbank_process, csdr_viewbank_*) through the host-thread emulation of the HIP sources (tests/emu) against one RefSpectrum in
view mode per slot (tests/viewbank_cases.py): every size, every walk, peak hold, hideDC, and the bit-for-bit properties and refusals.  No GPU
needed; the device runs the same cases in tests/test_gpu_viewbank.py."""
import ctypes as C
import os
import sys

import pytest

from tests import viewbank_cases as K

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


@pytest.mark.parametrize("F", K.SIZES)
def test_emu_viewbank_against_the_model(ctx, F):
    n, worst = K.check_against_model(ctx, F)
    assert n == sum(K.expected_counts(F).values()) and worst < K.TOL


@pytest.mark.parametrize("F", K.PEAK_SIZES)
def test_emu_viewbank_peak_hold(ctx, F):
    assert K.check_peak_hold(ctx, F) == 5 + 7 + 5


@pytest.mark.parametrize("F", (16, 256))
def test_emu_viewbank_hide_dc(ctx, F):
    assert K.check_hide_dc(ctx, F) == 12


@pytest.mark.parametrize("F", (16, 256))
def test_emu_viewbank_properties(ctx, F):
    K.check_properties(ctx, F)


@pytest.mark.parametrize("F", (32, 256))
def test_emu_viewbank_refusals(ctx, F):
    from cubicsdr_amd.engine import SDRPost
    post = SDRPost(ctx, 2400000, 4, 4096, 2)
    try:
        K.check_refusals(ctx, F, post)
    finally:
        post.close()
