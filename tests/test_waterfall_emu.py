"""The waterfall raster (kernels_waterfall.hpp, csdr_waterfall.hip) through the host-thread emulation of the HIP sources (tests/emu) against the numpy
model of tests/waterfall_cases.py, bit for bit: the quantiser over its special values and two whole binades in both layouts and with aligned and
unaligned sizes, the texture life cycle and the ring, the themed picture, and lines taken from a spectrum in HBM.  No GPU needed; the device runs
the same cases in tests/test_gpu_waterfall.py."""
import ctypes as C
import os
import sys

import pytest

from tests import waterfall_cases as K

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


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pairs"])
@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_emu_quantiser_specials(ctx, fft_size, pair):
    assert K.check_quantiser_specials(ctx, fft_size, pair) > 3000


@pytest.mark.parametrize("exponent", [-1, -8])
def test_emu_quantiser_whole_binade(ctx, exponent):
    """[0.5, 1) holds the clamp at 0.99; [2^-8, 2^-7) holds the first index step, 1 / 255"""
    assert K.check_quantiser_binade(ctx, exponent) == 1 << 23


def test_emu_worked_example(ctx):
    K.check_worked_example(ctx)


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pairs"])
@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_emu_life_cycle_and_ring(ctx, fft_size, pair):
    K.check_life_cycle(ctx, fft_size, pair)


@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_emu_rgba(ctx, fft_size):
    K.check_rgba(ctx, fft_size)


@pytest.mark.parametrize("hide_dc", [False, True], ids=["plain", "hide_dc"])
@pytest.mark.parametrize("fft_size,bandwidth", [(1024, 240000), (600, None)])
def test_emu_step_spec(ctx, fft_size, bandwidth, hide_dc):
    K.check_step_spec(ctx, fft_size, hide_dc, bandwidth)
