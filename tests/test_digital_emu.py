"""The digital decision kernel (kernels_digital.hpp) through the host-thread emulation of the HIP sources (tests/emu), against the reference
binary's modemcf / fskdem objects: every kind and constellation, FSK at several settings, and the refusals.  No GPU needed; the device runs
the same cases in tests/test_gpu_digital.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import digital_cases as D
from tests import digital_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))

pytestmark = pytest.mark.skipif(not O.available(), reason="the oracle (oracle/_ref) is not built: run __graft_entry__.build()")


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
def ref(tmp_path_factory):
    return O.shim(tmp_path_factory.mktemp("digital_shim"))


CONSTELLATIONS = [(k, c) for k in ("PSK", "DPSK", "ASK", "QAM", "BPSK", "QPSK", "OOK") for c in O.CONS[k]]


@pytest.mark.parametrize("kind,cons", CONSTELLATIONS)
def test_emu_digital_constellation(ctx, ref, kind, cons):
    D.check_constellation(ctx, ref, kind, cons)


@pytest.mark.parametrize("bps,k,bw", D.FSK_CASES)
def test_emu_digital_fsk(ctx, ref, bps, k, bw):
    D.check_fsk(ctx, ref, bps, k, bw)


@pytest.mark.parametrize("bps,k,bw", D.FSK_REFUSED)
def test_emu_digital_fsk_refused(ctx, ref, capfd, bps, k, bw):
    D.check_fsk_refused(ctx, ref, capfd, bps, k, bw)


def test_emu_digital_slot_needs_its_own_call(ctx):
    D.check_configure_routes(ctx)
