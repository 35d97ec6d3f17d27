"""The scope bank (scopebank_wave / scopebank_spectrum, csdr_scopebank_*) through the host-thread emulation of the HIP sources (tests/emu): the cases
of tests/scopebank_cases.py -- every size against the reference's own ScopeVisualProcessor, one per slot, and the byte-for-byte properties and
refusals against csdr_scope.  No GPU needed; the device runs the same cases in tests/test_gpu_scopebank.py."""
import ctypes as C
import os
import sys

import pytest

from tests import scopebank_cases as K

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


@pytest.mark.parametrize("L", K.SIZES)
def test_emu_scopebank_against_the_reference(ctx, L):
    n, worst = K.check_against_reference(ctx, L)
    assert n == 2 * 7 * K.FRAMES and worst < K.TOL


@pytest.mark.parametrize("L", K.BYTE_SIZES)
def test_emu_scopebank_properties(ctx, L):
    K.check_properties(ctx, L)


@pytest.mark.parametrize("L", K.BYTE_SIZES)
def test_emu_scopebank_refusals(ctx, L):
    from cubicsdr_amd.engine import DemodBank
    bank = DemodBank(ctx, 2, 1)
    try:
        K.check_refusals(ctx, L, bank)
    finally:
        bank.close()
