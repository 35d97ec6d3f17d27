"""csdr_design_density_cover (host only: the real library, no device) against the restatement of the rule in tests/density_oracle.py, on every item
of the shared cases (tests/density_cases.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import density_cases as K
from tests import density_oracle as D


@pytest.fixture(scope="module")
def design():
    from cubicsdr_amd.engine import design_density_cover
    return design_density_cover


def test_preconditions_of_the_cases(design):
    assert K.check_preconditions()
    # the header's example through the library, with every default of the Python layer: one frame, spectrum, layout 0, a dense stride
    it = K.CASES["header_example"]["steps"][0][0]
    assert K.mismatch(design(it["points"], 7, 10, 3), K.expected("header_example")[0][0][0]) is None


def test_density_palette_is_the_gradient():
    """engine.density_palette: csdr_design_gradient's 256 colours as bytes, round(255 v), with the caller's alpha"""
    from cubicsdr_amd.engine import density_palette, design_gradient
    stops = [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0]]
    pal = density_palette(stops)
    assert pal.shape == (256, 4) and pal.dtype == np.uint8 and (pal[:, 3] == 255).all()
    assert pal[0, :3].tolist() == [0, 0, 0] and pal[255, 0] == 255 and pal[255, 1] == 255         # (Gradient::generate stops one step short of the last stop)
    r, g, b = design_gradient(stops, 256)
    for k, ch in enumerate((r, g, b)):
        want = [min(255, max(0, int(float(v) * 255.0 + 0.5))) for v in ch]          # (Python floats: exact for float32 v times 255)
        assert pal[:, k].tolist() == want
    assert len({tuple(p) for p in pal[:, :3].tolist()}) > 100                       # a gradient, not a constant
    assert (density_palette(stops, alpha=200)[:, 3] == 200).all() and (density_palette(stops, alpha=200)[:, :3] == pal[:, :3]).all()


@pytest.mark.parametrize("name", list(K.CASES))
def test_design_cover_matches_the_rule(design, name):
    case = K.CASES[name]
    n_checked = 0
    for items in case["steps"]:
        for it in items:
            if it.get("points") is None:
                continue
            got = design(it["points"], case["W"], case["H"], it["n"], it["frames"], it.get("kind", "spectrum"), it.get("layout", 0), it.get("stride_floats"))
            want = D.item_cover(it, case["W"], case["H"])
            assert got.dtype == np.uint32 and K.mismatch(got, want) is None, (name, it["slot"], K.mismatch(got, want))
            n_checked += 1
    assert n_checked


def test_design_cover_refusals():
    import cubicsdr_amd.hip as H
    lib = H.lib()
    p = np.linspace(0, 1, 16).astype(np.float32)
    cov = np.full((4, 8), 77, np.uint32)
    pp, cp = p.ctypes.data_as(C.c_void_p), cov.ctypes.data_as(C.c_void_p)
    assert lib.csdr_design_density_cover(pp, 8, 0, 8, 2, 0, 8, 4, cp) == 0 and cov.sum() >= 16
    for args in ((pp, 8, 0, 8, 2, 2, 8, 4, cp), (pp, 8, 0, 8, 2, 3, 8, 4, cp), (pp, 8, 2, 8, 2, 0, 8, 4, cp), (pp, 8, 0, 7, 2, 0, 8, 4, cp),
                 (pp, 8, 1, 15, 1, 0, 8, 4, cp), (pp, -1, 0, 8, 2, 0, 8, 4, cp), (pp, 8, 0, 8, -1, 0, 8, 4, cp), (pp, 8, 0, 8, 2, 0, 1, 4, cp),
                 (pp, 8, 0, 8, 2, 0, 16385, 4, cp), (pp, 8, 0, 8, 2, 0, 8, 0, cp), (pp, 8, 0, 8, 2, 0, 8, 2049, cp), (pp, 8, 0, 8, 2, 0, 8, 4, None)):
        assert lib.csdr_design_density_cover(*args) == -1, args[1:8]
    assert lib.csdr_design_density_cover(pp, (1 << 21) + 1, 0, (1 << 21) + 1, 1, 0, 8, 4, cp) == -5
    assert lib.csdr_design_density_cover(None, 0, 0, 0, 0, 0, 8, 4, cp) == 0 and not cov.any()
