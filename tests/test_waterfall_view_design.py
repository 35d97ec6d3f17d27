"""The viewport's tap tables (csdr_design_view_columns / csdr_design_view_rows: design.hpp) from the real library, no device: against the numpy model
of tests/waterfall_view_cases.py, which is itself pinned against the reference's quad coordinates evaluated with fractions.Fraction; the PEAK ranges
as a partition of the ring; the refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import waterfall_view_cases as K

HALVES = (2, 3, 8, 15, 300, 1024, 32768)
WIDTHS = (2, 3, 4, 5, 16, 17, 601, 1920)
LINES = (2, 7, 12, 512)
HEIGHTS = tuple(range(1, 1081))
QUAD_HEIGHTS = tuple(range(1, 41)) + (255, 256, 257, 400, 511, 512, 513, 1023, 1024, 1025, 1080)      # (exact fractions are slow: a subset)


@pytest.fixture(scope="module")
def design():
    from cubicsdr_amd import build
    build.build(verbose=False)
    from cubicsdr_amd.engine import design_view_columns, design_view_rows
    return design_view_columns, design_view_rows


def same(got, want):
    for k in ("first", "count", "half"):
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:8])
    assert np.array_equal(got["frac"].view(np.uint32), want["frac"].view(np.uint32))


@pytest.mark.parametrize("half", HALVES)
def test_model_columns_are_the_reference_quads(half):
    for W in WIDTHS:
        K.check_taps_against_the_quads(half, W)


@pytest.mark.parametrize("lines", LINES)
def test_model_rows_are_the_reference_quads(lines):
    for Hh in QUAD_HEIGHTS:
        K.check_row_taps_against_the_quads(lines, Hh)


@pytest.mark.parametrize("half", HALVES)
def test_design_view_columns(design, half):
    for fft_size in (2 * half, 2 * half + 1):               # an odd fft_size: the last point is not drawn
        for W in WIDTHS + (min(2 * half, 16383), min(2 * half, 16383) + 1, 16384):
            for name, mode in K.MODES:
                got = design[0](fft_size, W, name)
                same(got, K.np_columns(fft_size, W, mode))
                n0 = W // 2
                assert not got["half"][:n0].any() and got["half"][n0:].all()
                if mode == K.LINEAR:
                    assert got["first"].min() >= 0 and got["first"].max() <= half - 2 and (got["frac"] < 1).all() and (got["frac"] >= 0).all()
                for part in (got[:n0], got[n0:]):
                    if mode == K.PEAK and part.size <= half:         # no bin is lost, none is read twice
                        assert part["first"][0] == 0 and part["first"][-1] + part["count"][-1] == half
                        assert np.array_equal(part["first"][1:], part["first"][:-1] + part["count"][:-1])
                    elif mode == K.PEAK:
                        assert (part["count"] == 1).all() and part["first"].max() == half - 1 and (np.diff(part["first"]) >= 0).all()


@pytest.mark.parametrize("lines", LINES)
def test_design_view_rows(design, lines):
    for Hh in HEIGHTS + (16384,):
        for name, mode in K.MODES:
            got = design[1](lines, Hh, name)
            same(got, K.np_rows(lines, Hh, mode))
            assert not got["half"].any()
            if mode == K.LINEAR:
                assert got["first"].min() >= -1 and got["first"].max() <= lines - 1 and (got["frac"] < 1).all() and (got["frac"] >= 0).all()
                if Hh == lines:
                    assert np.array_equal(got["first"], np.arange(lines)) and not got["frac"].any()
            elif Hh <= lines:                                # no line is lost, none is read twice
                assert got["first"][0] == 0 and got["first"][-1] + got["count"][-1] == lines
                assert np.array_equal(got["first"][1:], got["first"][:-1] + got["count"][:-1])
            else:
                assert (got["count"] == 1).all() and got["first"].max() == lines - 1


def test_design_view_refusals(design):
    import cubicsdr_amd.hip as H
    lib = H.lib()
    t = (H.ViewTap * 16)()
    before = bytes(t)
    for fft_size, W, mode in ((3, 16, 0), (2, 16, 1), (16, 1, 0), (16, 16385, 1), (16, 16, 2), (16, 16, -1), (-4, 16, 0)):
        assert lib.csdr_design_view_columns(fft_size, W, mode, t) == -1, (fft_size, W, mode)
    for lines, Hh, mode in ((1, 16, 0), ((1 << 20) + 1, 16, 1), (7, 0, 0), (7, 16385, 1), (7, 16, 2)):
        assert lib.csdr_design_view_rows(lines, Hh, mode, t) == -1, (lines, Hh, mode)
    assert lib.csdr_design_view_columns(16, 16, 0, None) == -1 and lib.csdr_design_view_rows(7, 16, 0, None) == -1
    assert bytes(t) == before
    assert C.sizeof(H.ViewTap) == 16 and H.ViewTap.frac.offset == 8 and H.ViewTap.half.offset == 12
