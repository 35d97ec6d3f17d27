"""The table-driven decision kernel (kernels_digital.hpp table_demod) through the host-thread emulation of the HIP sources (tests/emu), against the
reference binary's APSK / SQAM / V.29 / arb objects: all 16 built-in schemes and a user table.  No GPU needed; the device runs the same cases in
tests/test_gpu_table.py."""
import ctypes as C
import os
import sys

import pytest

from tests import table_cases as D
from tests import table_oracle as T

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))

pytestmark = pytest.mark.skipif(not T.available(), reason="the oracle (oracle/_ref) is not built: run __graft_entry__.build()")


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
def libs(tmp_path_factory):
    return T.Libs(tmp_path_factory.mktemp("table_shim"))


@pytest.mark.parametrize("name", T.NAMES)
def test_emu_table(ctx, libs, name):
    D.check_table(ctx, libs, name)


def test_emu_table_refusals(ctx, libs):
    D.check_refusals(ctx, libs)
