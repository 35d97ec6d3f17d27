"""The spectrum bank (specbank_process, csdr_specbank_*) through the host-thread emulation of the HIP sources (tests/emu) against one RefSpectrum per
slot (tests/specbank_cases.py): every size, every length sequence, peak hold, and the bit-for-bit properties and refusals.  No GPU needed; the device
runs the same cases in tests/test_gpu_specbank.py."""
import ctypes as C
import os
import sys

import pytest

from tests import specbank_cases as K

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
def test_emu_specbank_against_the_model(ctx, F):
    n, worst = K.check_against_model(ctx, F)
    assert n == 10 + 11 + 12 + 11 + 0 + 11 and worst < K.TOL


@pytest.mark.parametrize("F", K.PEAK_SIZES)
def test_emu_specbank_peak_hold(ctx, F):
    assert K.check_peak_hold(ctx, F) > 20


@pytest.mark.parametrize("F", (16, 32, 256))
def test_emu_specbank_properties(ctx, F):
    K.check_properties(ctx, F)


@pytest.mark.parametrize("F", (32, 256))
def test_emu_specbank_refusals(ctx, F):
    from cubicsdr_amd.engine import DemodBank
    bank = DemodBank(ctx, 2, 1)
    try:
        K.check_refusals(ctx, F, bank)
    finally:
        bank.close()
