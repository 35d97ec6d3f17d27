"""The native-sample-format ingest (kernels_io.hpp ingest_convert, csdr_io.hip's raw entry points) through the host-thread emulation of the HIP
sources (tests/emu): every component value of CS16 / CS8 / CU8 / CS12, every tail length, the ring, set_format and the refusals against the
header's arithmetic restated in numpy, bit for bit.  No GPU needed; the device runs the same cases in tests/test_gpu_raw_ingest.py."""
import ctypes as C
import os
import sys

import pytest

from tests import raw_ingest_cases as K

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


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_emu_every_component_value(ctx, fmt):
    assert K.check_every_value(ctx, fmt) >= 10


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_emu_every_length(ctx, fmt):
    assert K.check_lengths(ctx, fmt) == 203


def test_emu_cf32_passes_through(ctx):
    K.check_cf32_passes_through(ctx)


def test_emu_ring_contents(ctx):
    K.check_ring_contents(ctx)


def test_emu_ring_slot_tails(ctx):
    K.check_ring_slot_tails(ctx)


def test_emu_full_scale_is_required(ctx):
    K.check_full_scale_is_required(ctx)


def test_emu_set_format(ctx):
    K.check_set_format(ctx)


def test_emu_refusals(ctx):
    K.check_refusals(ctx)
