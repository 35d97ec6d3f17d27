"""The overlay bank on the device: every shared case (tests/overlay_cases.py) against the restated rule (tests/overlay_oracle.py), byte for byte --
base NULL, a host base, and a base a trace bank left in HBM --, the refusals, two sizes in a row and the picture left on the device and read
back."""
import numpy as np
import pytest

from tests import overlay_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ov(ctx):
    from cubicsdr_amd.engine import OverlayBank
    o = OverlayBank(ctx, max_tiles=16, max_prims=2048)
    o.set_font(K.FONT)
    yield o
    o.close()


@pytest.fixture(scope="module")
def tb(ctx):
    from cubicsdr_amd.engine import TraceBank
    t = TraceBank(ctx, max_items=4, max_points=4096)
    yield t
    t.close()


@pytest.mark.parametrize("name", list(K.CASES))
def test_case(ctx, ov, tb, name):
    K.check_case(ctx, ov, name, tb)


def test_refusals_change_nothing(ctx, ov):
    assert K.check_refusals(ctx, ov) >= 20


def test_two_sizes_in_a_row_and_the_device_view(ctx, ov):
    from cubicsdr_amd.engine import overlay_prims
    for name in ("w130_h70", "atlas_w7_h5", "w130_h70"):
        case = K.CASES[name]
        args = (overlay_prims(case["prims"]), case["runs"], case["W"], case["H"], case.get("cols", 1))
        want = K.expected(name, case["base"])
        assert ov.compose(*args, base=case["base"], fetch=False) is None
        p, w, h = ov.device_view()
        assert (h, w) == want.shape[:2]
        assert (K.download(ctx, p, want.shape) == want).all()
        assert (ov.compose(*args, base=case["base"]) == want).all()


def test_spectrum_annotations_on_the_device(ctx, ov):
    """engine.spectrum_annotations' list composed on the device against the oracle's list painted by the oracle"""
    from cubicsdr_amd.engine import spectrum_annotations
    from tests import overlay_oracle as O
    kw = dict(markers=[dict(freq=100200000, bandwidth=200000, label="[M] 10", flags=O.CENTERLINE | O.MUTED, rgb=(200, 50, 50))])
    prims = spectrum_annotations(130, 33, 100030000, 2400000, 1.0, 126.0, 1024, K.glyph_array(), K.LINE_HEIGHT, **kw)
    want = O.spectrum_annotations(130, 33, 100030000, 2400000, 1.0, 126.0, 1024, K.GLYPHS, K.LINE_HEIGHT, **kw)
    got = ov.compose(prims, [(0, len(prims))], 130, 33)
    assert len(prims) == len(want) and (got == O.atlas(want, [(0, len(want))], 130, 33, font=K.FONT)).all()
    assert np.count_nonzero(got) > 0
