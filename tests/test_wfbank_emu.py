"""The waterfall bank (kernels_wfbank.hpp, csdr_wfbank.hip) through the host-thread emulation of the HIP sources (tests/emu) against one PanelModel
per slot and one csdr_waterfall per slot, byte for byte (tests/wfbank_cases.py).  No GPU needed; the device runs the same cases in
tests/test_gpu_wfbank.py.  The emulation runs a host thread per work-item, so the largest pictures of the view cases are left to the device."""
import ctypes as C
import os
import sys

import pytest

from tests import wfbank_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
EMU_MAX_PIXELS = 40000


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


@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_emu_life_cycle(ctx, fft_size):
    assert K.check_life_cycle(ctx, fft_size) == 6


@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_emu_one_item_per_call_and_interleavings(ctx, fft_size):
    K.check_one_item_per_call(ctx, fft_size)


@pytest.mark.parametrize("fft_size", (16, 601))
def test_emu_slot_alone(ctx, fft_size):
    K.check_slot_alone(ctx, fft_size)


@pytest.mark.parametrize("fft_size", (30, 2048))
def test_emu_reset_slot(ctx, fft_size):
    K.check_reset_slot(ctx, fft_size)


def test_emu_setup_keeps_points(ctx):
    K.check_setup_keeps_points(ctx)


@pytest.mark.parametrize("fft_size", (2, 30, 2048))
def test_emu_refusals(ctx, fft_size):
    K.check_refusals(ctx, fft_size)


@pytest.mark.parametrize("mode", ["linear", "peak"])
@pytest.mark.parametrize("fft_size", K.VIEW_SIZES)
def test_emu_views(ctx, fft_size, mode):
    assert K.check_views(ctx, fft_size, mode, EMU_MAX_PIXELS) >= 12


@pytest.mark.parametrize("fft_size", K.VIEW_SIZES)
def test_emu_view_properties(ctx, fft_size):
    K.check_view_properties(ctx, fft_size)


@pytest.mark.parametrize("fft_size", (30, 2048))
def test_emu_against_one_waterfall_per_slot(ctx, fft_size):
    K.check_against_waterfalls(ctx, fft_size)
