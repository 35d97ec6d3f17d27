"""The squelch bank (squelch_scan / squelch_pack / squelch_pcm16, csdr_squelch_*) through the host-thread emulation of the HIP sources (tests/emu):
the cases of tests/squelch_cases.py -- both shapes against the checker bit for bit (the emulation's log10 is the host's), the recorder's bytes,
the reference's own DemodulatorThread where it is built, and the refusals against a twin.  No GPU needed; the device runs the same cases in
tests/test_gpu_squelch.py."""
import ctypes as C
import os
import sys

import pytest

from tests import squelch_cases as K

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


@pytest.mark.parametrize("n_slots", K.SHAPES)
def test_emu_squelch_against_the_checker(ctx, n_slots):
    n = K.check_scenario(ctx, n_slots, exact=True)
    assert n == n_slots * sum(K.CALLS) - K.CALLS[K.ABSENT[1]]


def test_emu_squelch_against_the_reference_thread(ctx):
    import oracle.ref_modems as RM
    if not RM.demodthread_available():
        pytest.skip("oracle/_ref/libref_demodthread.so is built only where the reference is")
    assert K.check_against_demodthread(ctx, exact=True) == 168


def test_emu_squelch_refusals(ctx):
    from cubicsdr_amd.engine import Context, DemodBank
    other = Context(0)
    bank, other_bank = DemodBank(ctx, 2, 1), DemodBank(other, 2, 1)
    try:
        K.check_refusals(ctx, bank, other_bank)
    finally:
        bank.close(); other_bank.close(); other.close()
