"""The waterfall's viewport (wf_view_linear / wf_view_peak, csdr_waterfall_render_view) through the host-thread emulation of the HIP sources
(tests/emu) against the numpy model of tests/waterfall_view_cases.py, bit for bit: every width, height, mode and ring state of the cases, the
equalities with fetch_rgba, and the refusals.  No GPU needed; the device runs the same cases in tests/test_gpu_waterfall_view.py."""
import ctypes as C
import os
import sys

import pytest

from tests import waterfall_view_cases as K

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


@pytest.mark.parametrize("lines", K.LINES)
@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_emu_views(ctx, fft_size, lines):
    assert K.check_views(ctx, fft_size, lines) == (7 + 2 + 2) * 5 * 2


@pytest.mark.parametrize("fft_size,lines", [(16, 7), (30, 12), (601, 7), (2048, 12)])
def test_emu_view_properties(ctx, fft_size, lines):
    K.check_view_properties(ctx, fft_size, lines)


def test_emu_wide_footprints(ctx):
    K.check_wide_footprints(ctx)
