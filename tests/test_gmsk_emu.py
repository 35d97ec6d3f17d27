"""The GMSK kernels (kernels_digital.hpp gmsk_phase / gmsk_decide) through the host-thread emulation of the HIP sources (tests/emu), against the
reference binary's gmskdem: modulated signals with noise and a carrier offset, pure noise, split streams, exact zeros and the refusals.  No GPU
needed; the device runs the same cases in tests/test_gpu_gmsk.py."""
import ctypes as C
import os
import sys

import pytest

from tests import gmsk_cases as K
from tests import gmsk_oracle as G

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))

pytestmark = pytest.mark.skipif(not G.available(), reason="the oracle (oracle/_ref) is not built: run __graft_entry__.build()")


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
    return G.shim(tmp_path_factory.mktemp("gmsk_shim"))


@pytest.mark.parametrize("k,m,bt", K.SETTINGS)
def test_emu_gmsk_modulated(ctx, ref, k, m, bt):
    K.check_modulated(ctx, ref, k, m, bt)


@pytest.mark.parametrize("k,m,bt", K.SETTINGS[:4])
def test_emu_gmsk_noise(ctx, ref, k, m, bt):
    K.check_noise(ctx, ref, k, m, bt)


@pytest.mark.parametrize("k,m,bt", K.SETTINGS[:4])
def test_emu_gmsk_split_stream(ctx, ref, k, m, bt):
    K.check_split(ctx, ref, k, m, bt)


@pytest.mark.parametrize("k,m,bt", [(4, 3, 0.3), (2, 1, 0.5), (5, 2, 0.25)])
def test_emu_gmsk_signed_zeros(ctx, ref, k, m, bt):
    K.check_signed_zeros(ctx, ref, k, m, bt)


def test_emu_gmsk_refused(ctx, ref):
    K.check_refused(ctx, ref)
