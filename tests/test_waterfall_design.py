"""csdr_design_gradient (host only: the real library, no device) against the numpy restatement of Gradient::generate in tests/waterfall_cases.py, bit for
bit: 2, 3, 5, 6, 7, 256 and 257 stops -- chunk remainders that are zero and not zero, stops outside [0, 1] -- other lengths, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import cubicsdr_amd.hip as H
from tests import waterfall_cases as K


@pytest.fixture(scope="module", autouse=True)
def lib():
    from cubicsdr_amd import build
    build.build(verbose=False)
    return H.lib()


@pytest.mark.parametrize("n_colors", [2, 3, 5, 6, 7, 256, 257])
def test_gradient_256(n_colors):
    want = K.check_design_gradient(n_colors)
    assert want.shape == (256, 3) and want.min() >= 0.0 and want.max() <= 1.0
    if n_colors >= 5:
        assert want.min() == 0.0 and want.max() == 1.0          # the clamp was at work on both sides


@pytest.mark.parametrize("n_colors,length", [(2, 1), (2, 2), (3, 2), (4, 10), (7, 100), (11, 10), (5, 1000)])
def test_gradient_other_lengths(n_colors, length):
    K.check_design_gradient(n_colors, length, seed=9)


def test_gradient_remainders():
    assert 256 % 5 == 1 and 256 % 4 == 0 and 256 % 6 == 4     # 6, 5 and 7 stops: the last chunk is longer; 2, 3, 5, 257 stops: it is not
    g = K.np_gradient([[0, 0, 0], [1, 1, 1]], 256)
    assert g[0, 0] == 0.0 and g[255, 0] == np.float32(255) / np.float32(256)


def test_gradient_refusals(lib):
    out = [np.empty(256, np.float32) for _ in range(3)]
    ptr = [o.ctypes.data_as(C.c_void_p) for o in out]
    stops = np.zeros((300, 3), np.float32)
    s = stops.ctypes.data_as(C.c_void_p)
    assert lib.csdr_design_gradient(s, 2, 256, *ptr) == 0
    assert lib.csdr_design_gradient(s, 257, 256, *ptr) == 0
    for n in (-1, 0, 1, 258, 300):
        assert lib.csdr_design_gradient(s, n, 256, *ptr) == -1, n
    assert lib.csdr_design_gradient(s, 12, 10, *ptr) == -1
    assert lib.csdr_design_gradient(s, 2, 0, *ptr) == -1
    assert lib.csdr_design_gradient(None, 2, 256, *ptr) == -1
    assert lib.csdr_design_gradient(s, 2, 256, None, ptr[1], ptr[2]) == -1
    assert b"gradient" in lib.csdr_last_error()
